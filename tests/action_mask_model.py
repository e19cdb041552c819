"""Test helper: the numpy specification of the action mask of constrained generation (csrc/gi_mask.hip,
``graphinvent_amd.sampler.ActionConstraint`` / ``mask_actions``).  The device must match it exactly: which columns of an
APD row are admissible is decided in integers, and a masked row holds the input's bits or ``-inf``.

Columns of a row of width ``W = N A + N Fe + 1`` (``A = prod(dim_f_add[1:])``), as ``gi_sample_actions`` decodes them:
``add(i, rem)`` at ``i A + rem`` with ``rem`` ravelled over ``dim_f_add[1:]`` (the node-feature groups first — atom
type, formal charge, [implicit H], [whatever follows] — the bond type ``f`` last), ``connect(i, f)`` at
``N A + i Fe + f``, ``terminate`` at ``W - 1``.

The state of a graph with ``n`` atoms is WELL-FORMED when the labelled read (tests/valence_model.judge) sets none of
its malformed bits and no self-loop bit.  For such a state and an atom ``i < n``:
``budget2(i) = 2 vmax(type_i, charge_i) - o2_i - 2 s_i`` with ``o2_i`` twice the bond-order sum, ``vmax`` the largest
allowed valence (-1: the combination has none) and ``s_i`` the stored hydrogen count (0 without an implicit-H segment).

Structural rules, always:  ``add(i, ...)``: ``n < N``, and ``i == 0`` if ``n == 0`` else ``i < n``;  ``connect(i, f)``:
``n >= 2``, ``i < n - 1``, no set entry in ``edges[i, n - 1, :]``;  ``terminate``: ``n >= 1`` or ``allow_empty``.
Valence rules, for a well-formed state under ``valence=True``:  ``add(i, type, charge, [h], ..., f)`` with ``n >= 1``:
``order2[f] <= budget2(i)`` and ``order2[f] + 2 h <= 2 vmax(type, charge)``; with ``n == 0``: ``2 h <= 2 vmax(type,
charge)``, any ``f``;  ``connect(i, f)``: ``order2[f] <= budget2(i)`` and ``order2[f] <= budget2(n - 1)``.
A state that is not well-formed gets the structural rules and the status bit ``MASK_STRUCTURAL``.

``status`` = the malformed and self-loop bits of the read, plus ``MASK_STRUCTURAL`` when any of them is set."""
import numpy as np

from tests import canon_model as CM
from tests import valence_model as VM

MASK_STRUCTURAL = 1 << 20
ILL_FORMED = VM.MALFORMED | VM.VAL_SELF_LOOP


def dims(dim_f_add):
    """-> (N, groups, Fe, A, W)."""
    N, sub = int(dim_f_add[0]), [int(x) for x in dim_f_add[1:]]
    A = int(np.prod(sub, dtype=np.int64))
    return N, sub[:-1], sub[-1], A, N * A + N * sub[-1] + 1


def read_status(nodes, edges, n_given, rules):
    """The labelled read's bits that make a state ill-formed, and n clamped to [0, N]."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N = nodes.shape[0]
    A, C, H = rules.groups
    status, n = CM.status_of(nodes, edges, n_given)
    nz_n, nz_e = nodes != 0, edges != 0
    off = [0, A, A + C, A + C + H]
    for s in range(3 if H else 2):
        if (nz_n[:n, off[s]:off[s + 1]].sum(axis=1) != 1).any():
            status |= VM.MOL_ONEHOT
    if (nz_e.sum(axis=2)[~np.eye(N, dtype=bool)] > 1).any():
        status |= VM.MOL_MULTI_BOND
    if nz_e[np.arange(N), np.arange(N)].any():
        status |= VM.VAL_SELF_LOOP
    return status, n


def vmax_table(rules):
    """[types, charges]: the largest allowed valence, -1 where there is none."""
    return np.array([[max(v) if len(v) else -1 for v in row] for row in rules.allowed], np.int64)


def admissible(nodes, edges, n_given, rules, dim_f_add, allow_empty=False, valence=True):
    """One graph -> (allowed bool [W], status)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N, groups, Fe, A, W = dims(dim_f_add)
    T, C, H = rules.groups
    assert nodes.shape == (N, sum(groups)) and edges.shape == (N, N, Fe) and len(rules.order2) == Fe
    assert groups[0] == T and groups[1] == C and (H == 0 or groups[2] == H)
    status, n = read_status(nodes, edges, n_given, rules)
    sound = not status & ILL_FORMED
    if not sound:
        status |= MASK_STRUCTURAL
    nz_n, nz_e = nodes != 0, edges != 0
    order2 = np.array(rules.order2, np.int64)
    Q = A // Fe
    idx = np.unravel_index(np.arange(Q), groups)
    i = np.arange(N)
    # structural
    add_ok = np.zeros(N, bool)
    if n < N:
        add_ok = (i == 0) if n == 0 else (i < n)
    conn_ok = np.zeros(N, bool)
    if n >= 2:
        conn_ok = (i < n - 1) & ~nz_e[:, n - 1, :].any(axis=1)
    add = np.broadcast_to(add_ok[:, None, None], (N, Q, Fe)).copy()
    conn = np.broadcast_to(conn_ok[:, None], (N, Fe)).copy()
    term = n >= 1 or bool(allow_empty)
    if valence and sound:
        vmax = vmax_table(rules)
        hval = np.array(rules.h_values, np.int64)[idx[2]] if H else np.zeros(Q, np.int64)
        lim2 = 2 * vmax[idx[0], idx[1]] - 2 * hval                      # [Q]: what the new atom can still take
        budget2 = np.zeros(N, np.int64)
        for a in range(n):
            t = int(np.flatnonzero(nz_n[a, :T])[0])
            c = int(np.flatnonzero(nz_n[a, T:T + C])[0])
            s = int(rules.h_values[int(np.flatnonzero(nz_n[a, T + C:T + C + H])[0])]) if H else 0
            o2 = int((nz_e[a].sum(axis=0) * order2).sum())
            budget2[a] = 2 * vmax[t, c] - o2 - 2 * s
        if n == 0:
            add &= (lim2 >= 0)[None, :, None]
        else:
            add &= order2[None, None, :] <= budget2[:, None, None]
            add &= order2[None, None, :] <= lim2[None, :, None]
            conn &= order2[None, :] <= budget2[:, None]
            conn &= order2[None, :] <= budget2[n - 1]
    return np.concatenate([add.reshape(-1), conn.reshape(-1), [term]]), status


def pack_bits(allowed):
    """bool [..., W] -> uint32 [..., ceil(W / 32)]: column j is bit ``j & 31`` of word ``j >> 5``."""
    allowed = np.asarray(allowed, bool)
    W = allowed.shape[-1]
    pad = np.zeros(allowed.shape[:-1] + (-(-W // 32) * 32,), bool)
    pad[..., :W] = allowed
    return np.packbits(pad.reshape(pad.shape[:-1] + (-1, 32)), axis=-1, bitorder="little").view("<u4")[..., 0]


def mask_batch(logits, nodes, edges, n_nodes, rules, dim_f_add, allow_empty=False, valence=True):
    """Batch model of ``mask_actions`` -> dict(masked [B, W] fp32: the input's bits or -inf, allowed bool [B, W],
    n_admissible / status [B] int32, bits uint32 [B, ceil(W / 32)])."""
    logits = np.asarray(logits, np.float32)
    B, W = logits.shape
    allowed = np.zeros((B, W), bool)
    status = np.zeros(B, np.int32)
    for b in range(B):
        allowed[b], status[b] = admissible(nodes[b], edges[b], n_nodes[b], rules, dim_f_add, allow_empty, valence)
    raw = logits.view(np.uint32).copy()
    raw[~allowed] = np.float32(-np.inf).view(np.uint32)
    return dict(masked=raw.view(np.float32), allowed=allowed, n_admissible=allowed.sum(axis=1).astype(np.int32),
                status=status, bits=pack_bits(allowed))


def removed_mass(logits, allowed):
    """fp64: 1 - (softmax mass of the admissible columns), per row (0 for a row without positive mass)."""
    z = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(z - z.max(axis=1, keepdims=True))
    e = np.where(np.isnan(e), 0.0, e)
    tot = e.sum(axis=1)
    kept = (e * allowed).sum(axis=1)
    return np.where(tot > 0, 1.0 - kept / np.where(tot > 0, tot, 1.0), 0.0)


def apply_action(nodes, edges, n, j, dim_f_add):
    """Column j applied to one graph as ``gi_grow_graphs`` applies it (tests/grow_oracle.grow_round); returns the new
    n, or -1 for terminate."""
    N, groups, Fe, A, W = dims(dim_f_add)
    if j == W - 1:
        return -1
    offs = np.concatenate([[0], np.cumsum(groups)[:-1]])
    if j < N * A:
        i, rem = divmod(j, A)
        q, f = divmod(rem, Fe)
        sub = np.unravel_index(q, groups)
        for k in range(len(groups)):
            nodes[n, offs[k] + sub[k]] = 1
        if n != 0:
            edges[i, n, f] = edges[n, i, f] = 1
        return n + 1
    i, f = divmod(j - N * A, Fe)
    edges[i, n - 1, f] = edges[n - 1, i, f] = 1
    return n


def action_bound(n, vmax_sum):
    """An upper bound on the actions of a terminated molecule of n atoms grown under the mask from the empty graph:
    n adds, at most ``sum vmax / 2 - (n - 1)`` connects (every bond takes 2 of the half-valences, n - 1 bonds come
    with the adds), one terminate."""
    return n + vmax_sum // 2 - (n - 1) + 1
