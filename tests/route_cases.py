"""Test helper: molecules at the seams of csrc/gi_route.hip (node counts around the 64-lane loops, step codes that use
every bit of the 16-bit pair word, row pitches below and across the 16-byte pieces, molecule counts around the scan's
1024-entry chunks, 1 and 4 feature segments, APD sums of exactly 127 and 128) and a REPLAY check of expanded rows.

The replay decodes every row's hot APD index as an action and applies it to the row's graph: it must give the row
before.  It knows nothing about the removal order (which node goes next, type-major neighbour lists, step numbers),
so it cannot share a mistake with tests/routes_model.py or with the kernels' closed form.  No GPU code is imported."""
import functools

import numpy as np

from tests import reorder_model as OM


def modes(name):
    """How the GPU test runs a case: 2(b) unmerged only, the piece cases a third time with `n_rows` given."""
    if name == "steps-fe4":
        return ("unmerged",)
    return ("unmerged", "merged", "n_rows") if name.startswith("piece-") else ("unmerged", "merged")


class Case:
    """A batch of molecules with its APD dims and the ways the GPU test runs it."""

    def __init__(self, name, nodes, edges, seg):
        self.name, self.modes = name, modes(name)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.int8)
        self.edges = np.ascontiguousarray(edges, dtype=np.int8)
        self.M, self.N, self.Fn = self.nodes.shape
        self.Fe = self.edges.shape[3]
        self.seg = [int(s) for s in seg]
        self.add, self.conn = [self.N] + self.seg + [self.Fe], [self.N, self.Fe]
        self.width = int(np.prod(self.add)) + self.N * self.Fe + 1
        self.apd_itemsize = 1 if self.M <= 127 else 4


# ---- the replay ---------------------------------------------------------------------------------------------
def replay(rn, re, hot, mol_nodes, mol_edges, add, conn):
    """Check the rows (rn [L, N, Fn], re [L, N, N, Fe], hot [L]) of ONE molecule; raises AssertionError.  Returns the
    bond steps it decoded, [(k, i, j, t)]: row k's action bonds node i (the last node of row k - 1) to j < i by t."""
    add, Fe, N = [int(x) for x in add], int(add[-1]), int(add[0])
    bounds = np.concatenate([[0], np.cumsum(add[1:-1])])
    n_add = int(np.prod(add))
    width = n_add + int(np.prod(conn)) + 1
    L = len(hot)
    n_edges = int(np.asarray(mol_edges).any(axis=2).sum()) // 2
    assert L == len(rn) == len(re) == n_edges + 2, f"{L} rows for {n_edges} bonds"
    assert not rn[L - 1].any() and not re[L - 1].any(), "the last row is not empty"
    assert int(hot[0]) == width - 1, "row 0 does not terminate"
    assert np.array_equal(rn[0], mol_nodes) and np.array_equal(re[0], mol_edges), "row 0 is not the molecule"
    steps = []
    for k in range(1, L):
        h = int(hot[k])
        assert 0 <= h < width - 1, f"row {k}: hot index {h} is no add / connect action"
        gn, ge = np.array(rn[k]), np.array(re[k])
        present = gn.any(axis=1)
        n = int(present.sum())
        assert present[:n].all(), f"row {k}: nodes are not a prefix"
        if h < n_add:
            idx = [int(x) for x in np.unravel_index(h, add)]
            j, feats, t = idx[0], idx[1:-1], idx[-1]
            assert n < N, f"row {k}: no room for another node"
            for s, q in enumerate(feats):
                gn[n, bounds[s] + q] = 1
            if n == 0:
                assert j == 0 and t == 0, f"row {k}: the first node's action is not f_add[0, .., 0]"
            else:
                assert j < n, f"row {k}: a new node bonded to node {j} of {n}"
                ge[n, j, t] = ge[j, n, t] = 1
                steps.append((k, n, j, t))
        else:
            j, t = divmod(h - n_add, Fe)
            last = n - 1
            assert last >= 1 and j < last and not ge[last, j].any(), f"row {k}: connect ({last}, {j}) is not possible"
            ge[last, j, t] = ge[j, last, t] = 1
            steps.append((k, last, j, t))
        assert np.array_equal(gn, rn[k - 1]) and np.array_equal(ge, re[k - 1]), \
            f"row {k}: its action does not lead to row {k - 1}"
    return steps


def replay_batch(rn, re, hot, row_mol, mol_nodes, mol_edges, add, conn):
    """The replay of every molecule of unmerged rows; returns the bond steps per molecule."""
    row_mol = np.asarray(row_mol)
    M = len(mol_nodes)
    assert (np.diff(row_mol) >= 0).all() and (len(row_mol) == 0 or (row_mol[0] >= 0 and row_mol[-1] < M))
    at = np.searchsorted(row_mol, np.arange(M + 1))
    return [replay(rn[at[m]:at[m + 1]], re[at[m]:at[m + 1]], hot[at[m]:at[m + 1]], mol_nodes[m], mol_edges[m],
                   add, conn) for m in range(M)]


def well_formed(nodes, edges, seg):
    """The input contract of routes.expand, asserted: int8 0 / 1, one-hot per segment on a zero-padded node prefix,
    symmetric edges with one type per pair and none on padding or the diagonal, a lower neighbour for every i > 0."""
    assert nodes.dtype == np.int8 and edges.dtype == np.int8
    assert set(np.unique(nodes)) <= {0, 1} and set(np.unique(edges)) <= {0, 1}
    bounds = np.concatenate([[0], np.cumsum(seg)])
    assert bounds[-1] == nodes.shape[2]
    for m in range(nodes.shape[0]):
        n = int(nodes[m].any(axis=1).sum())
        assert n >= 1 and not nodes[m, n:].any()
        for s in range(len(seg)):
            assert (nodes[m, :n, bounds[s]:bounds[s + 1]].sum(axis=1) == 1).all()
        assert np.array_equal(edges[m], edges[m].transpose(1, 0, 2))
        adj = edges[m].sum(axis=2)
        assert adj.max(initial=0) <= 1 and not adj[n:].any() and not np.diagonal(adj).any()
        assert (np.tril(adj, -1)[1:n].sum(axis=1) >= 1).all()


# ---- generators ---------------------------------------------------------------------------------------------
def _features(rng, n, N, seg):
    nodes = np.zeros((N, sum(seg)), dtype=np.int8)
    at = 0
    for s in seg:
        nodes[np.arange(n), at + rng.integers(0, s, size=n)] = 1
        at += s
    return nodes


class _Types:
    """Bond types: cycling 0, 1, .., Fe - 1, 0, .. or drawn."""

    def __init__(self, Fe, rng=None):
        self.Fe, self.rng, self.c = Fe, rng, 0

    def __call__(self):
        if self.rng is not None:
            return int(self.rng.integers(0, self.Fe))
        self.c += 1
        return (self.c - 1) % self.Fe


def _bond(edges, i, j, t):
    edges[i, j, t] = edges[j, i, t] = 1


def tree_molecule(rng, n, N, seg, Fe, closures=0, cycle=False, top=None):
    """A random tree on nodes 0 .. n - 1 (every node bonded to a lower one) plus `closures` ring closures among the
    first `top` nodes (default: all)."""
    nodes = _features(rng, n, N, seg)
    edges = np.zeros((N, N, Fe), dtype=np.int8)
    typ = _Types(Fe, None if cycle else rng)
    for i in range(1, n):
        _bond(edges, i, int(rng.integers(0, i)), typ())
    top = n if top is None else top
    for _ in range(closures):
        for _ in range(100):
            i, j = (int(x) for x in rng.integers(0, top, size=2))
            if i != j and not edges[i, j].any():
                _bond(edges, i, j, typ())
                break
    return nodes, edges


def truncated(nodes, edges, n):
    nodes, edges = nodes.copy(), edges.copy()
    nodes[n:] = 0
    edges[n:] = 0
    edges[:, n:] = 0
    return nodes, edges


def _stack(mols):
    return np.stack([a for a, _ in mols]), np.stack([b for _, b in mols])


def random_batch(rng, M, N, seg, Fe, closures=2):
    """M random molecules of 1 .. N nodes; the first has N."""
    return _stack([tree_molecule(rng, N if m == 0 else int(rng.integers(1, N + 1)), N, seg, Fe,
                                 closures=int(rng.integers(0, closures + 1))) for m in range(M)])


SEAM_N = (1, 2, 63, 64, 65, 127, 128)


def node_seams(N):
    """Case 1.  Molecule 3 (N >= 65): a chain in which node 64 has the lower neighbours 63, 10 and 20, and, where node
    64 is not itself the last node, the last node N - 1 has the lower neighbours N - 2, 64, 3 and 67 (3 and 67 are
    the same lane of the 64-lane loop, in different trips)."""
    rng = np.random.default_rng(1000 + N)
    seg, Fe = [3, 2], 3
    full = tree_molecule(rng, N, N, seg, Fe, closures=N // 4, cycle=True)
    mols = [full, truncated(*full, max(N - 1, 1)), tree_molecule(rng, 1, N, seg, Fe)]
    if N >= 65:
        nodes = _features(rng, N, N, seg)
        edges = np.zeros((N, N, Fe), dtype=np.int8)
        typ = _Types(Fe)
        for i in range(1, N):
            _bond(edges, i, i - 1, typ())
        for j in (10, 20):
            _bond(edges, 64, j, typ())
        if N - 1 > 67:
            for j in (64, 3, 67):
                _bond(edges, N - 1, j, typ())
        mols.append((nodes, edges))
    return Case(f"nodes-{N}", *_stack(mols), seg)


def complete_128():
    """Case 2(a): K_128 with one bond type: 8130 rows, the last step is 8129 (bits 0 .. 12 of the step all used)."""
    N = 128
    nodes = np.zeros((1, N, 2), dtype=np.int8)
    nodes[0, :, 0] = nodes[0, :, 1] = 1
    edges = np.ones((1, N, N, 1), dtype=np.int8)
    edges[0, np.arange(N), np.arange(N)] = 0
    return Case("k128", nodes, edges, [1, 1])


STEPS_FE4_DENSITY = 0.53


def steps_fe4():
    """Case 2(b): N = 128, Fe = 4, a chain plus every other pair with probability 0.53, type (i + j) mod 4."""
    N, Fe = 128, 4
    rng = np.random.default_rng(2004)
    nodes = np.zeros((1, N, 2), dtype=np.int8)
    nodes[0, :, 0] = nodes[0, :, 1] = 1
    edges = np.zeros((1, N, N, Fe), dtype=np.int8)
    take = np.tril(rng.random((N, N)) < STEPS_FE4_DENSITY, -1)
    for i in range(1, N):
        for j in range(i):
            if take[i, j] or j == i - 1:
                _bond(edges[0], i, j, (i + j) % Fe)
    return Case("steps-fe4", nodes, edges, [1, 1])


CODES_TYPE0 = (0, 5, 33, 63, 64, 65, 90, 101, 126)          # node 127's type-0 neighbours
CODES_TYPED = {t: 8 * t + 64 * (t % 2) for t in range(1, 8)}  # its one neighbour of each type 1 .. 7


def codes_fe8():
    """Case 2(c): N = 128, Fe = 8, 600 bonds of all eight types.  Node 127 (first step 1) has one bond of each type
    7 .. 1, which take steps 1 .. 7, and nine type-0 bonds, which take steps 8 .. 16: the code 8 of a type-0 bond
    equals the `type + 1` marker of type 7, and an ascending type sweep would hand the type-0 bonds the codes 1 .. 9,
    eight of which are markers of the other types the node carries."""
    N, Fe, seg = 128, 8, [2, 1]
    rng = np.random.default_rng(2008)
    nodes, edges = tree_molecule(rng, N - 1, N, seg, Fe, closures=600 - 126 - 16, cycle=True)
    nodes[N - 1] = _features(rng, 1, 1, seg)[0]
    for j in CODES_TYPE0:
        _bond(edges, N - 1, j, 0)
    for t, j in CODES_TYPED.items():
        _bond(edges, N - 1, j, t)
    return Case("codes-fe8", nodes[None], edges[None], seg)


PIECE_SHAPES = ((1, [2], 1), (2, [2, 1], 1), (3, [3, 2], 2), (5, [2, 1], 3), (7, [4, 3, 2], 5))
PIECE_M = (5, 130)


def pieces(shape, M):
    """Case 3: row pitches below 16 bytes, odd APD widths; int8 (M = 5) and fp32 (M = 130) APDs."""
    N, seg, Fe = PIECE_SHAPES[shape]
    rng = np.random.default_rng(3000 + 10 * shape + M)
    return Case(f"piece-{shape}-{M}", *random_batch(rng, M, N, seg, Fe), seg)


SCAN_M = (1023, 1024, 1025, 2049)


def scan_seams(M):
    """Case 4: M molecules drawn from six distinct N = 3 molecules."""
    rng = np.random.default_rng(4000)
    seg, Fe = [3, 2], 3
    kinds, seen = [], set()
    while len(kinds) < 6:
        mol = tree_molecule(rng, int(rng.integers(1, 4)), 3, seg, Fe, closures=1)
        key = mol[0].tobytes() + mol[1].tobytes()
        if key not in seen:
            seen.add(key)
            kinds.append(mol)
    nodes, edges = _stack(kinds)
    pick = np.random.default_rng(4000 + M).integers(0, 6, size=M)
    return Case(f"scan-{M}", nodes[pick], edges[pick], seg)


def scan_distinct():
    """Case 4, last item: distinct random N = 5 molecules whose merged rows outnumber one scan chunk."""
    rng = np.random.default_rng(4500)
    seg, Fe = [3, 2], 3
    mols, seen = [], set()
    while len(mols) < 400:
        mol = tree_molecule(rng, int(rng.integers(4, 6)), 5, seg, Fe, closures=int(rng.integers(0, 4)))
        key = mol[0].tobytes() + mol[1].tobytes()
        if key not in seen:
            seen.add(key)
            mols.append(mol)
    return Case("scan-distinct", *_stack(mols), seg)


SEGMENTS = ([6], [2, 3, 2, 2])


def segments(which):
    """Case 5: one and four feature segments at N = 9, Fe = 3, M = 40."""
    seg = SEGMENTS[which]
    rng = np.random.default_rng(5000 + which)
    return Case(f"seg-{len(seg)}", *random_batch(rng, 40, 9, seg, 3), seg)


def sum_boundary(M):
    """Case 6: M copies of one molecule."""
    rng = np.random.default_rng(6000)
    nodes, edges = tree_molecule(rng, 4, 4, [3, 2], 3, closures=1)
    return Case(f"sum-{M}", np.repeat(nodes[None], M, axis=0), np.repeat(edges[None], M, axis=0), [3, 2])


_BUILDERS = {}
_BUILDERS.update({f"nodes-{N}": functools.partial(node_seams, N) for N in SEAM_N})
_BUILDERS.update({"k128": complete_128, "steps-fe4": steps_fe4, "codes-fe8": codes_fe8})
_BUILDERS.update({f"piece-{s}-{M}": functools.partial(pieces, s, M) for s in range(len(PIECE_SHAPES)) for M in PIECE_M})
_BUILDERS.update({f"scan-{M}": functools.partial(scan_seams, M) for M in SCAN_M})
_BUILDERS.update({"scan-distinct": scan_distinct, "seg-1": functools.partial(segments, 0),
                  "seg-4": functools.partial(segments, 1), "sum-127": functools.partial(sum_boundary, 127),
                  "sum-128": functools.partial(sum_boundary, 128)})
NAMES = tuple(_BUILDERS)


def case(name) -> Case:
    return _BUILDERS[name]()


# ---- case 7: reorder, then expand ---------------------------------------------------------------------------
REORDER_N, REORDER_ROUTES = (65, 128), ("bfs", "dfs")
REORDER_SEG, REORDER_FE = [4], 3


def reorder_inputs(N, route):
    """Three connected molecules in a random input order (N, N - 1 and about N / 2 nodes) and a ranking each."""
    rng = np.random.default_rng(7000 + N + (route == "dfs"))
    mols = [OM.random_molecule(rng, n, N, REORDER_SEG[0], REORDER_FE, kind, extra=N // 8)
            for n, kind in ((N, "tree"), (N - 1, "ring"), (N // 2 + 1, "tree"))]
    nodes, edges = _stack(mols)
    rank = np.zeros((3, N), dtype=np.int32)
    for m in range(3):
        n = OM.n_nodes(nodes[m])
        rank[m, :n] = rng.permutation(n)
    return nodes, edges, rank
