"""
Inputs for graph_compact (graphinvent_amd/csrc/gi_compact.hip) at the limits of its axes — node count, bond types,
slot count, feature classes, feature width — and a checker of its index arrays against their DEFINITION, so that
the numpy model `tests/ref_dataflow.py::compact` is itself checked by something that is not a second implementation
of the same formulas.  The generators and the checker are plain numpy; `_compact_case` is the GPU comparison the
kernel tests share.

Every generator is deterministic and returns int8 ``(nodes [B,N,Fn], edges [B,N,N,Fe])``; edges[b, i, j, t] = 1 is
the edge i <- j of bond type t.
"""
from __future__ import annotations

import numpy as np

from tests import ref_dataflow as D

DEV = "cuda"
P0_MAX = 256           # GI_P0_MAX_CLASSES
P0_MAX_FN = 62         # widest feature row the pass-0 shortcut takes


# ------------------------------------------------------------------------------------------------
# the GPU comparison (moved here from tests/test_kernels_gpu.py)
# ------------------------------------------------------------------------------------------------
def to_dev(a: np.ndarray, in_dtype: str = "f32"):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if in_dtype == "i8" else t.float()).to(DEV)


def _compact_case(n8, e8, H=16, nodedup=False, in_dtype="f32"):
    """ops.compact against D.compact, bit-exact.  in_dtype: what the kernels are handed, "f32" or "i8" (the
    <signed char> instantiations of count and fill).  Returns (graph, hx0, reference dict)."""
    from graphinvent_amd import ops
    assert in_dtype in ("f32", "i8")
    ref = D.compact(n8, e8, nodedup=nodedup)
    g, hx0 = ops.compact(to_dev(n8, in_dtype), to_dev(e8, in_dtype), H, class_csr=True, nodedup=nodedup)
    if nodedup:      # every slot its own row, every edge its own message row, no pass-0 rows
        assert (g.S, g.U, g.D0) == (n8.shape[0] * n8.shape[1], g.E, 0)
        assert np.array_equal(g.mu_off.cpu().numpy(), np.arange(g.E + 1))
    assert (g.S, g.E, g.U) == (ref["S"], ref["E"], ref["U"])
    assert list(g.Ut) == np.diff(ref["type_off"]).tolist()
    for name in ("cidx", "slot_of", "u_src", "in_perm", "mu_off", "mu_dst", "mu_slot", "out_perm",
                 "type_off"):
        got = getattr(g, name).cpu().numpy()
        assert np.array_equal(got, ref[name]), name            # integer work: bit-exact
    for name in ("seg_off", "src_off"):                        # [R + 1] = [S + 2] entries
        assert np.array_equal(getattr(g, name).cpu().numpy(), ref[name]), name
    # pass-0 rows: (feature class, bond type) pairs, their gather rows and the edge-count matrix
    assert g.D0 == ref["D0"]
    if g.D0:
        assert np.array_equal(g.type_off0.cpu().numpy(), ref["type_off0"])
        assert np.array_equal(g.d_src.cpu().numpy(), ref["d_src"])
        assert np.array_equal(g.cmat.cpu().numpy()[:, :g.D0], ref["cmat"])
        assert float(g.cmat.sum()) == g.E
        # AttentionGGNN's pass 0: edge slot -> pass-0 row, and the row -> edge slots CSR (stable order)
        assert g.class_csr
        for name in ("e2d", "cls_off", "cls_edges"):
            assert np.array_equal(getattr(g, name).cpu().numpy(), ref[name]), name
    assert np.array_equal(g.node_mask.cpu().numpy(), ref["node_mask"].astype(np.int32))
    B, N, Fn = n8.shape
    x = np.zeros((g.S + 1, hx0.shape[1]), dtype=np.float32)
    rows = n8.reshape(B * N, Fn)[ref["slot_of"]].astype(np.float32)
    x[:g.S, :Fn] = rows
    x[:g.S, H:H + Fn] = rows
    assert np.array_equal(hx0.cpu().numpy(), x)
    return g, hx0, ref


# ------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------
#: seven distinct non-zero 0/1 feature rows of width 8
FEATURE_ROWS = np.array([[1, 0, 0, 0, 0, 1, 0, 0],
                         [0, 1, 0, 0, 0, 1, 0, 0],
                         [0, 0, 1, 0, 0, 1, 0, 0],
                         [0, 0, 0, 1, 0, 1, 0, 0],
                         [1, 0, 0, 0, 0, 0, 1, 0],
                         [0, 1, 0, 0, 0, 0, 0, 1],
                         [0, 0, 0, 0, 1, 0, 0, 1]], dtype=np.int8)


def _bond(edges, b, i, j, t):
    edges[b, i, j, t] = 1
    edges[b, j, i, t] = 1


def _feature(nodes, b, slots):
    slots = np.asarray(slots, dtype=np.int64)
    nodes[b, slots] = FEATURE_ROWS[(slots + 3 * b) % len(FEATURE_ROWS)]


def seam_graphs(N: int, Fe: int):
    """B = 4, Fn = 8.
    0: the path 0-1-..-(N-1), bond (k, k+1) of type k % Fe, closed by (0, N-1) (N >= 3: below that the pair is the
       path's own bond or a single atom) and, for N > 65, by (0, 64) and (63, N-1): bonds across the 64-bit word seam
       of a row and of a column;
    1: a star centred on slot N-1 (its row and column have bits in both words, the leaves have the last bit set);
    2: random sparse symmetric bonds on slots [0, N-3), then slot N-3 with all-zero features and ONE incoming edge
       (N-3 <- 0, nothing back), slot N-2 featured without any bond, slot N-1 empty (as far as N has room for them);
    3: empty."""
    rng = np.random.default_rng(7919 * N + Fe)
    nodes = np.zeros((4, N, 8), dtype=np.int8)
    edges = np.zeros((4, N, N, Fe), dtype=np.int8)
    _feature(nodes, 0, np.arange(N))
    for k in range(N - 1):
        _bond(edges, 0, k, k + 1, k % Fe)
    closures = [(0, N - 1)] if N >= 3 else []
    if N > 65:
        closures += [(0, 64), (63, N - 1)]
    for i, j in closures:
        _bond(edges, 0, i, j, (i + j) % Fe)
    _feature(nodes, 1, np.arange(N))
    for k in range(N - 1):
        _bond(edges, 1, k, N - 1, k % Fe)
    M = N - 1                                   # slots graph 2 may use
    if M >= 1:
        _feature(nodes, 2, [M - 1])             # a featured atom with no bond
    n_rand = M - 2 if M >= 3 else max(M - 1, 0)
    _feature(nodes, 2, np.arange(n_rand))
    if n_rand >= 2:
        p = min(1.0, 3.0 / n_rand)
        for i in range(n_rand):
            for j in range(i + 1, n_rand):
                if rng.random() < p:
                    _bond(edges, 2, i, j, int(rng.integers(Fe)))
        if not edges[2].any():
            _bond(edges, 2, 0, n_rand - 1, 0)
    if M >= 3:
        edges[2, M - 2, 0, (M - 2) % Fe] = 1    # one-way: (M-2) <- 0, into an all-zero feature row
    return nodes, edges


def all_types_graph(N: int, Fe: int):
    """B = 2, Fn = 8.  0: the complete graph with every bond type on every pair (each cell holds the mask 2**Fe - 1:
    N (N-1) Fe edges); 1: a single bond of type Fe-1 between slots 0 and N-1."""
    nodes = np.zeros((2, N, 8), dtype=np.int8)
    edges = np.zeros((2, N, N, Fe), dtype=np.int8)
    _feature(nodes, 0, np.arange(N))
    edges[0] = 1
    edges[0, np.arange(N), np.arange(N)] = 0
    _feature(nodes, 1, [0, N - 1])
    _bond(edges, 1, 0, N - 1, Fe - 1)
    return nodes, edges


def class_batch(Q: int, Fe: int, all_types: bool = False):
    """Q graphs of two atoms, Fn = 9: both atoms of graph b carry the 9-bit pattern of b + 1 and are joined by one
    bond of type b % Fe (all Fe types with all_types) — Q feature classes, Q (or Q Fe) pass-0 rows."""
    assert 1 <= Q < 512
    nodes = np.zeros((Q, 2, 9), dtype=np.int8)
    edges = np.zeros((Q, 2, 2, Fe), dtype=np.int8)
    for b in range(Q):
        nodes[b, :, :] = [((b + 1) >> f) & 1 for f in range(9)]
        for t in (range(Fe) if all_types else [b % Fe]):
            _bond(edges, b, 0, 1, t)
    return nodes, edges


def wide_feature_bits(Fn: int):
    """The set feature bits of wide_feature_batch's three atoms: between them bits 0, 31, 32 and Fn-1 (those that
    exist), and above 33 features three patterns that differ ONLY in bits >= 32."""
    a = [0, 31]
    b = a + [32] if Fn > 32 else [0]
    c = a + [Fn - 1] if Fn > 33 else ([0, 32] if Fn == 33 else [31])
    return a, b, c


def wide_feature_batch(Fn: int):
    """B = 1, N = 3, Fe = 3: the path A - B - C with bond types 0 and 1, feature bits see wide_feature_bits."""
    nodes = np.zeros((1, 3, Fn), dtype=np.int8)
    edges = np.zeros((1, 3, 3, 3), dtype=np.int8)
    for slot, bits in enumerate(wide_feature_bits(Fn)):
        nodes[0, slot, bits] = 1
    _bond(edges, 0, 0, 1, 0)
    _bond(edges, 0, 1, 2, 1)
    return nodes, edges


def slot_count_batch(B: int, N: int):
    """Fn = 8, Fe = 3: every slot is an atom with probability 1/2 and the atoms of a graph form a path with random
    bond types; the first and the last graph are full paths, so the first and the last slot of the batch count."""
    rng = np.random.default_rng(104729 * B + N)
    nodes = np.zeros((B, N, 8), dtype=np.int8)
    edges = np.zeros((B, N, N, 3), dtype=np.int8)
    for b in range(B):
        atoms = np.arange(N) if b in (0, B - 1) else np.nonzero(rng.random(N) < 0.5)[0]
        nodes[b, atoms] = FEATURE_ROWS[rng.integers(len(FEATURE_ROWS), size=len(atoms))]
        for i, j in zip(atoms[:-1], atoms[1:]):
            _bond(edges, b, i, j, int(rng.integers(3)))
    return nodes, edges


def edge_count_batch(E: int, classes: int = 1, Fe: int = 3):
    """Exactly E directed edges from path molecules of at most 9 atoms (16 edges each), a shorter path for the rest
    and, for an odd E, one graph with a single one-way edge.  classes = 1: one feature row and bond type 0 everywhere
    (one pass-0 row); otherwise slot i of graph b is of class (i + b) % classes and bond k of type k % Fe, so that
    every (bond type, class) pair occurs once the batch has a few graphs."""
    N = 9
    bonds_of = []
    r = E
    while r >= 2:
        bonds_of.append(min(N - 1, r // 2))
        r -= 2 * bonds_of[-1]
    B = len(bonds_of) + r
    nodes = np.zeros((B, N, 8), dtype=np.int8)
    edges = np.zeros((B, N, N, Fe), dtype=np.int8)
    for b in range(B):
        nb = bonds_of[b] if b < len(bonds_of) else 1
        nodes[b, :nb + 1] = FEATURE_ROWS[(np.arange(nb + 1) + b) % classes]
        if b < len(bonds_of):
            for k in range(nb):
                _bond(edges, b, k, k + 1, k % Fe if classes > 1 else 0)
        else:
            edges[b, 0, 1, 0] = 1                # the odd edge: 0 <- 1 only
    return nodes, edges


def path_batch(G: int, N: int, Fe: int = 3):
    """G identical path graphs over all N slots (bond k of type k % Fe), one feature row everywhere."""
    nodes = np.zeros((G, N, 8), dtype=np.int8)
    edges = np.zeros((G, N, N, Fe), dtype=np.int8)
    nodes[:] = FEATURE_ROWS[0]
    for k in range(N - 1):
        edges[:, k, k + 1, k % Fe] = 1
        edges[:, k + 1, k, k % Fe] = 1
    return nodes, edges


# ------------------------------------------------------------------------------------------------
# the definitional checker
# ------------------------------------------------------------------------------------------------
def _segments_are(perm, off, group_of, n_groups, total, name):
    """perm[off[g] : off[g+1]] lists exactly the items of group g in ascending order, for every g."""
    off = np.asarray(off, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    assert off.shape == (n_groups + 1,) and perm.shape == (total,), name
    assert off[0] == 0 and off[-1] == total and np.all(np.diff(off) >= 0), name
    assert np.array_equal(np.sort(perm), np.arange(total)), name + ": not a permutation"
    owner = np.repeat(np.arange(n_groups), np.diff(off))
    assert np.array_equal(group_of[perm], owner), name + ": item in another group's segment"
    same = owner[1:] == owner[:-1]
    assert np.all(perm[1:][same] > perm[:-1][same]), name + ": segment not ascending"


def check_invariants(nodes, edges, ref, nodedup: bool = False):
    """A result dict of graph_compact (the keys of D.compact) against the definition of its arrays."""
    B, N, Fn = nodes.shape
    Fe = edges.shape[3]
    ns = B * N
    S, E, U, D0 = ref["S"], ref["E"], ref["U"], ref["D0"]
    bonds = edges == 1
    eb, ei, ej, et = (a.astype(np.int64) for a in np.nonzero(bonds))      # set entries in row-major order
    dst_slot, src_slot = eb * N + ei, eb * N + ej
    indeg = np.bincount(dst_slot, minlength=ns)
    outdeg = np.bincount(src_slot, minlength=ns)
    feat = nodes.reshape(ns, Fn)
    active = np.ones(ns, dtype=bool) if nodedup else (feat != 0).any(1) | (indeg > 0) | (outdeg > 0)
    # ---- compact rows ------------------------------------------------------------------------------
    cidx, slot_of = ref["cidx"].astype(np.int64), ref["slot_of"].astype(np.int64)
    assert S == int(active.sum()) and E == eb.size
    assert cidx.shape == (ns,) and slot_of.shape == (S,)
    assert np.all(cidx[~active] == S)
    assert np.array_equal(slot_of[cidx[active]], np.nonzero(active)[0])
    assert np.all(np.diff(slot_of) > 0)                                   # rows in ascending slot order
    assert np.array_equal(ref["node_mask"].astype(np.int64), (indeg > 0).astype(np.int64))
    multi = bool(np.any(bonds.sum(3) > 1))
    assert ref["err"] == (int(np.any((edges != 0) & ~bonds)) | (8 if multi else 0))
    # ---- dst-CSR: the slot of an entry is its row-major rank k ------------------------------------------
    k = np.arange(E)
    seg_off = ref["seg_off"].astype(np.int64)
    assert seg_off.shape == (S + 2,) and seg_off[S] == E and seg_off[S + 1] == E
    c_dst = cidx[dst_slot]
    assert np.all(seg_off[c_dst] <= k) and np.all(k < seg_off[c_dst + 1])
    same = dst_slot[1:] == dst_slot[:-1]                                  # inside a segment k ascends in (j, t)
    assert np.all((ej[1:] * Fe + et[1:])[same] > (ej[:-1] * Fe + et[:-1])[same])
    assert np.array_equal(np.diff(seg_off[:S + 1]), indeg[slot_of])
    # ---- message rows ------------------------------------------------------------------------------
    in_perm, u_src = ref["in_perm"].astype(np.int64), ref["u_src"].astype(np.int64)
    type_off = ref["type_off"].astype(np.int64)
    assert in_perm.shape == (E,) and u_src.shape == (U,) and type_off.shape == (Fe + 1,)
    assert type_off[0] == 0 and type_off[Fe] == U
    if E:
        assert in_perm.min() >= 0 and in_perm.max() < U
    assert np.array_equal(u_src[in_perm], cidx[src_slot])
    assert np.all(type_off[et] <= in_perm) and np.all(in_perm < type_off[et + 1])
    # one row per (bond type, source slot) pair — per edge without sharing —, rows ordered by that key
    ukey = (et * ns + src_slot) * (N if nodedup else 1) + (ei if nodedup else 0)
    key_of = np.full(U, -1, dtype=np.int64)
    key_of[in_perm] = ukey
    assert np.all(key_of >= 0) and np.array_equal(key_of[in_perm], ukey)
    assert np.all(np.diff(key_of) > 0)
    assert U == (E if nodedup else np.unique(ukey).size)
    # ---- message CSR: the edges k of every message row, ascending, with their destination rows -------------
    _segments_are(ref["mu_slot"], ref["mu_off"], in_perm, U, E, "mu_slot")
    assert np.array_equal(ref["mu_dst"].astype(np.int64), c_dst[ref["mu_slot"].astype(np.int64)])
    # ---- source CSR: the message rows of every source row, by ascending type (= ascending row id) ----------
    src_off = ref["src_off"].astype(np.int64)
    assert src_off.shape == (S + 2,) and src_off[S + 1] == U
    _segments_are(ref["out_perm"], src_off[:S + 2], u_src, S + 1, U, "out_perm")
    # ---- pass-0 rows ---------------------------------------------------------------------------------
    pattern = np.zeros(ns, dtype=np.uint64)
    for f in range(min(Fn, 64)):
        pattern |= (feat[:, f] == 1).astype(np.uint64) << np.uint64(f)
    binary = bool(np.all((feat == 0) | (feat == 1)))
    n_classes = np.unique(pattern[src_slot]).size
    expect_on = binary and Fn <= P0_MAX_FN and E > 0 and not nodedup and n_classes <= P0_MAX
    assert (D0 > 0) == expect_on
    if D0 == 0:
        assert ref["cmat"] is None
        return
    e2d, d_src, type_off0 = ref["e2d"].astype(np.int64), ref["d_src"].astype(np.int64), ref["type_off0"]
    cmat = ref["cmat"]
    assert e2d.shape == (E,) and d_src.shape == (D0,) and cmat.shape == (S + 1, D0)
    assert e2d.min() >= 0 and e2d.max() < D0 and np.unique(e2d).size == D0
    # a pass-0 row = a (bond type, pattern of the source) pair; rows ordered by type, then unsigned pattern
    pairs = sorted(set(zip(et.tolist(), pattern[src_slot].tolist())))
    assert len(pairs) == D0
    row_of = {p: d for d, p in enumerate(pairs)}
    assert np.array_equal(e2d, np.array([row_of[p] for p in zip(et.tolist(), pattern[src_slot].tolist())]))
    assert cmat.sum() == E
    counts = np.zeros((S + 1, D0), dtype=np.int64)
    np.add.at(counts, (c_dst, e2d), 1)
    assert np.array_equal(cmat, counts.astype(cmat.dtype))
    _segments_are(ref["cls_edges"], ref["cls_off"], e2d, D0, E, "cls_edges")
    lowest = np.full(D0, S + 1, dtype=np.int64)
    np.minimum.at(lowest, e2d, cidx[src_slot])
    assert np.array_equal(d_src, lowest)
    assert type_off0.shape == (Fe + 1,) and type_off0[0] == 0 and type_off0[Fe] == D0
    d_type = np.array([p[0] for p in pairs])
    assert np.all(type_off0[d_type] <= np.arange(D0)) and np.all(np.arange(D0) < type_off0[d_type + 1])

