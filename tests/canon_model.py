"""Test helper: the numpy / pure-Python specification of molecule identity on the device (csrc/gi_canon.hip,
``graphinvent_amd.analyze.canonical`` / ``unique`` / ``SeenSet``): canonical node order by colour refinement with
individualisation (no backtracking), the canonical molecule, its 128-bit key, uniqueness inside a call with a mask, and
the key-only seen-set across calls.  The device must match it bit for bit.

The algorithm (n = the molecule's node count, rows compared as byte strings, all sums modulo 2**64):

  initial colour  col_i = #{j < n : row_j < row_i}
  refinement      h_i = sum over (t, j) with a bond of type t between i and j of mix64(t << 32 | col_j);
                  col'_i = #{j : (col_j, h_j) < (col_i, h_i)}; repeated until the number of distinct colours stops growing
  individualise   while colours repeat: in the non-singleton cell of smallest colour r the member of lowest input index
                  keeps r, the others get r + 1; refine again
  order           nodes by ascending final colour; form = nodes[order], edges[order][:, order], zero padded
  key             k0 = mix64(n) + sum mix64(1 << 40 | a Fn + f) + sum mix64(2 << 40 | (a N + b) Fe + t) over the set
                  entries (a, f) / (a, b, t) of the form; k1 the same with the tags 3, 4, 5; a zero word becomes 1

A molecule that fails a check (status bits, ``lib.MOL_*`` plus the two below) keeps the identity order over all N
slots, a zero form and a key made of its index; it is never equal to anything."""
import bisect

import numpy as np

MASK = (1 << 64) - 1
MOL_BOND_PAST_N, MOL_VALUE = 2, 8                            # lib.MOL_*
MOL_ASYMMETRIC, MOL_NODE_PAST_N = 32, 64                     # lib.MOL_ASYMMETRIC, lib.MOL_NODE_PAST_N
SEEN_FULL = 1                                                # lib.SEEN_FULL


def mix64(x: int) -> int:
    """The splitmix64 step of csrc/gi_route.hip / gi_reorder.hip / gi_canon.hip (64-bit wrap-around)."""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def derived_n(nodes) -> int:
    """n_nodes = None: the number of LEADING node rows with a set entry."""
    any_row = np.asarray(nodes).any(axis=1)
    return int(len(any_row) if any_row.all() else np.argmin(any_row))


def status_of(nodes, edges, n_given) -> tuple:
    """-> (status bits, n clamped to [0, N])."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N = nodes.shape[0]
    status = 0
    n = derived_n(nodes) if n_given is None else int(n_given)
    if n < 0 or n > N:
        status |= MOL_NODE_PAST_N
        n = min(max(n, 0), N)
    if ((nodes != 0) & (nodes != 1)).any() or ((edges != 0) & (edges != 1)).any():
        status |= MOL_VALUE
    if (nodes[n:] != 0).any():
        status |= MOL_NODE_PAST_N
    if (edges[n:] != 0).any() or (edges[:, n:] != 0).any():
        status |= MOL_BOND_PAST_N
    if not np.array_equal(edges != 0, (edges != 0).transpose(1, 0, 2)):
        status |= MOL_ASYMMETRIC
    return status, n


def _ranks(keys):
    """rank_i = #{j : key_j < key_i}, and the number of distinct keys."""
    s = sorted(keys)
    return [bisect.bisect_left(s, k) for k in keys], len(set(keys))


def canonical_order(nodes, edges, n, stats=None):
    """The canonical order (input index of every canonical position) of a well-formed molecule of n nodes."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    rows = [nodes[i].astype(np.uint8).tobytes() for i in range(n)]
    nbr = [[(int(t), int(j)) for j, t in zip(*np.nonzero(edges[i, :n]))] for i in range(n)]
    col, cells = _ranks(rows)
    rounds = indiv = 0
    while True:
        while cells < n:
            h = [sum(mix64((t << 32) | col[j]) for t, j in nbr[i]) & MASK for i in range(n)]
            col, c2 = _ranks(list(zip(col, h)))
            rounds += 1
            if c2 == cells:
                break
            cells = c2
        if cells == n:
            break
        seen, r = set(), None
        for c in sorted(col):                                  # the smallest colour that repeats
            if c in seen:
                r = c
                break
            seen.add(c)
        keep = col.index(r)
        col = [c + 1 if (c == r and i != keep) else c for i, c in enumerate(col)]
        cells += 1
        indiv += 1
    if stats is not None:
        stats.update(rounds=rounds, individualisations=indiv)
    return sorted(range(n), key=lambda i: col[i])


def form_of(nodes, edges, order):
    """nodes[order], edges[order][:, order], zero padded to N, int8."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    out_n = np.zeros(nodes.shape, dtype=np.int8)
    out_e = np.zeros(edges.shape, dtype=np.int8)
    o = np.asarray(order, dtype=np.int64)
    if len(o):
        out_n[:len(o)] = nodes[o]
        out_e[:len(o), :len(o)] = edges[o][:, o]
    return out_n, out_e


def _nonzero_word(x):
    return x if x else 1


def key_of(form_n, form_e, n):
    N, Fn = form_n.shape
    Fe = form_e.shape[2]
    k0, k1 = mix64(n), mix64((3 << 40) | n)
    for x in np.flatnonzero(form_n.reshape(-1)).tolist():
        k0 += mix64((1 << 40) | x)
        k1 += mix64((4 << 40) | x)
    for y in np.flatnonzero(form_e.reshape(-1)).tolist():
        k0 += mix64((2 << 40) | y)
        k1 += mix64((5 << 40) | y)
    return _nonzero_word(k0 & MASK), _nonzero_word(k1 & MASK)


def failed_key(g):
    return _nonzero_word(mix64((6 << 40) | g)), _nonzero_word(mix64((7 << 40) | g))


def canonical(nodes, edges, n_nodes=None):
    """Batch model of ``analyze.canonical(..., want_molecules=True)``: a dict of order / rank [G, N] int32 (-1 past
    n), key [G, 2] uint64, status [G] int32, nodes / edges (int8, the canonical molecules)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    G, N = nodes.shape[:2]
    out = dict(order=np.full((G, N), -1, np.int32), rank=np.full((G, N), -1, np.int32),
               key=np.zeros((G, 2), np.uint64), status=np.zeros(G, np.int32),
               nodes=np.zeros(nodes.shape, np.int8), edges=np.zeros(edges.shape, np.int8))
    for g in range(G):
        status, n = status_of(nodes[g], edges[g], None if n_nodes is None else n_nodes[g])
        out["status"][g] = status
        if status:
            out["order"][g] = out["rank"][g] = np.arange(N)
            out["key"][g] = failed_key(g)
            continue
        order = canonical_order(nodes[g], edges[g], n)
        out["order"][g, :n] = order
        out["rank"][g, order] = np.arange(n)
        out["nodes"][g], out["edges"][g] = form_of(nodes[g].astype(np.int8), edges[g].astype(np.int8), order)
        out["key"][g] = key_of(out["nodes"][g], out["edges"][g], n)
    return out


def unique(canon, mask=None):
    """Model of ``gi_mol_unique`` over ``canonical``'s result -> (unique fp32 [G], rep int32 [G], counts int32 [3]):
    equal means equal key AND equal canonical bytes, both molecules well-formed."""
    G = len(canon["status"])
    mask = np.ones(G, bool) if mask is None else np.asarray(mask) != 0
    rep = np.full(G, -1, np.int32)
    uniq = np.ones(G, np.float32)
    first = {}
    for g in range(G):
        if not mask[g]:
            continue
        if canon["status"][g]:
            rep[g] = g
            continue
        ident = (tuple(canon["key"][g].tolist()), canon["nodes"][g].tobytes(), canon["edges"][g].tobytes())
        rep[g] = first.setdefault(ident, g)
        if rep[g] != g:
            uniq[g] = 0.0
    counts = np.array([int(np.bitwise_or.reduce(canon["status"])) if G else 0, int(mask.sum()),
                       int((rep == np.arange(G)).sum())], np.int32)
    return uniq, rep, counts


class SeenSet:
    """Model of ``analyze.SeenSet``: 128-bit keys only, a fixed capacity.  (Which keys of an overflowing call still
    get in is decided by timing on the device and by position here; everything else is the device's result.)"""

    def __init__(self, capacity):
        self.capacity, self.keys, self.full = capacity, set(), False

    def add(self, canon, rep, mask=None):
        G = len(rep)
        new = np.zeros(G, np.int32)
        for g in range(G):
            if rep[g] != g:
                continue
            if canon["status"][g]:
                new[g] = 1                                       # never equal to anything, never stored
                continue
            k = tuple(canon["key"][g].tolist())
            if k in self.keys:
                continue
            new[g] = 1
            if len(self.keys) < self.capacity:
                self.keys.add(k)
            else:
                self.full = True
        return new

    def count(self):
        return len(self.keys)


# ---- generators for the tests -------------------------------------------------------------------------------
def permute(nodes, edges, perm):
    """The molecule with its first len(perm) nodes in the order `perm` (position a holds input node perm[a])."""
    return form_of(nodes, edges, perm)


def from_bonds(N, Fn, Fe, labels, bonds):
    """A padded molecule from node labels (the set feature of every node) and bonds (i, j, type)."""
    nodes, edges = np.zeros((N, Fn), np.int8), np.zeros((N, N, Fe), np.int8)
    for i, f in enumerate(labels):
        nodes[i, f] = 1
    for i, j, t in bonds:
        edges[i, j, t] = edges[j, i, t] = 1
    return nodes, edges


def ring(n, t=0):
    return [(i, (i + 1) % n, t) for i in range(n)] if n > 2 else [(0, 1, t)][:n - 1]


def path(n, t=0):
    return [(i, i + 1, t) for i in range(n - 1)]


def complete(n, t=0):
    return [(i, j, t) for i in range(n) for j in range(i + 1, n)]
