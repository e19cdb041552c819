"""Golden decoding routes from the UNMODIFIED reference ``MolecularGraph.PreprocessingGraph``
(``get_decoding_route_state``, ``get_decoding_APD``, ``truncate_graph``; MolecularGraph.py:463-555, 635-732).

Runs only where the reference checkout is (``python tests/golden/make_golden_routes.py [path/to/graphinvent]``).
``MolecularGraph.py`` imports ``rdkit`` and ``util`` at module level.  ``rdkit`` is not installed here and none of the
methods under test touches it, so empty stub modules stand in for ``rdkit``, ``rdkit.Chem`` and
``rdkit.Chem.rdmolfiles``.  ``util`` is tried first as it is, under further stubs (``rdkit.RDLogger``,
``parameters.constants``); it builds a tensorboard writer at import and needs matplotlib, so where that fails — it
does in the build container: this script prints which way it went and records it in the file — a stub ``util``
module supplies ``get_feature_vector_indices`` alone, the cumulative sizes of the feature segments taken from the
``constants`` this script builds (what util.py:26-47 computes from the same constants).  Nothing of the reference is
patched: the ``int(np.nonzero(...)[0])`` at MolecularGraph.py:511-513 converts a 1-element array, which numpy still
accepts with a deprecation warning.

Graphs are bare ``PreprocessingGraph`` instances (``object.__new__``, then ``constants``, ``node_features``,
``edge_features`` and ``n_nodes``), i.e. the state after ``node_remap`` and ``pad_graph_representation``; every
``get_decoding_route_state(k)``, k = 0 .. n_edges + 1, is recorded.

Output ``golden_routes.npz``: per configuration ``c`` the input molecules (``c::mol_nodes``, ``c::mol_edges``),
``c::dim_f_add`` / ``c::dim_f_conn``, every route row's ``c::rows_nodes`` / ``c::rows_edges`` (int8), the hot index of
its APD ``c::hot`` (unmerged APDs are one-hot; the script asserts that), and ``c::row_mol`` / ``c::row_step``.

Configurations:
  gdb13    N = 13, 5 atom types x 3 charges, 3 bond types: the 20 whole molecules of the shipped fixtures
           gdb13_1K-debug_{train,valid} (the rows whose f_term is set), then 120 seeded synthetic ones — a single
           atom, two atoms, chains and trees, ring closures that leave the last node with degree 2, 3 and 4, last
           nodes whose bonds have mixed types so that the type-major neighbour order differs from the index order
  arom5    N = 13, Fe = 4 (aromatic), implicit-H segment: dim_f_add has rank 5
  chiral6  N = 40, Fe = 4, implicit-H and chirality segments: dim_f_add has rank 6
"""
import os
import sys
import tempfile
import types
import warnings
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/graphinvent"

CURRENT = {"seg": None}          # feature segment sizes of the configuration being recorded (the stub util reads it)


def load_reference():
    class Stub(types.ModuleType):                            # any name (rdkit.Chem.Mol, .Atom, ... in annotations)
        def __getattr__(self, attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return object

    for name in ("rdkit", "rdkit.Chem", "rdkit.Chem.rdmolfiles"):
        sys.modules[name] = Stub(name)
    sys.modules["rdkit"].Chem = sys.modules["rdkit.Chem"]
    sys.modules["rdkit"].RDLogger = types.SimpleNamespace(DisableLog=lambda *a: None)
    sys.modules["rdkit.Chem"].rdmolfiles = sys.modules["rdkit.Chem.rdmolfiles"]
    sys.path.insert(0, REF)
    real_util = False
    saved = {k: sys.modules.get(k) for k in ("parameters", "parameters.constants")}
    try:
        pc = types.ModuleType("parameters.constants")
        pc.constants = types.SimpleNamespace(tensorboard_dir=tempfile.mkdtemp(), use_explicit_H=False, ignore_H=False,
                                             use_chirality=False, n_atom_types=0, n_formal_charge=0, n_imp_H=0,
                                             n_chirality=0, job_type="preprocess")
        sys.modules["parameters"] = types.ModuleType("parameters")
        sys.modules["parameters.constants"] = pc
        import util
        real_util = util.__file__.startswith(REF)
    except Exception as e:                                   # noqa: BLE001 — whatever util wants and is not here
        print(f"util does not import under stubs ({type(e).__name__}: {e}); supplying get_feature_vector_indices")
        for k, v in saved.items():
            sys.modules.pop(k, None) if v is None else sys.modules.__setitem__(k, v)
        stub = types.ModuleType("util")
        stub.get_feature_vector_indices = lambda: np.cumsum(CURRENT["seg"]).tolist()
        sys.modules["util"] = stub
    import MolecularGraph
    assert MolecularGraph.__file__.startswith(REF)
    return MolecularGraph, real_util


def set_segments(seg, real_util):
    CURRENT["seg"] = list(seg)
    if real_util:                                            # the real function reads parameters.constants
        c = sys.modules["parameters.constants"].constants
        c.n_atom_types, c.n_formal_charge = seg[0], seg[1]
        c.ignore_H = len(seg) < 3
        c.n_imp_H = seg[2] if len(seg) > 2 else 0
        c.use_chirality = len(seg) > 3
        c.n_chirality = seg[3] if len(seg) > 3 else 0


# ---- inputs ---------------------------------------------------------------------------------------------
def synthetic(rng, n, N, seg, Fe, extra, last_degree=None, mixed_last=False, chain=False):
    """A padded molecule in a BFS-like order: node i > 0 bonds to a lower node, plus `extra` ring closures."""
    nodes = np.zeros((N, sum(seg)), dtype=np.int8)
    edges = np.zeros((N, N, Fe), dtype=np.int8)
    off = np.concatenate([[0], np.cumsum(seg)])
    for i in range(n):
        for s, size in enumerate(seg):
            nodes[i, off[s] + rng.integers(0, size)] = 1

    def bond(i, j, t):
        edges[i, j, t] = edges[j, i, t] = 1

    for i in range(1, n):
        bond(i, i - 1 if chain else int(rng.integers(0, i)), int(rng.integers(0, Fe)))
    for _ in range(extra):
        i, j = (int(x) for x in rng.integers(0, n, size=2))
        if i != j and not edges[i, j].any():
            bond(i, j, int(rng.integers(0, Fe)))
    last = n - 1
    if last_degree is not None and last >= last_degree:
        edges[last] = 0
        edges[:, last] = 0
        picks = rng.choice(last, size=last_degree, replace=False)
        types_ = rng.integers(0, Fe, size=last_degree)
        if mixed_last:                                       # the highest index gets the lowest type: type-major order
            picks = np.sort(picks)                           # ends on a different node than index order would
            types_ = np.sort(types_ if len(set(types_)) > 1 else np.arange(last_degree) % Fe)[::-1]
        for j, t in zip(picks, types_):
            bond(last, int(j), int(t))
    return nodes, edges


def gdb13_molecules():
    mols = []
    for split in ("train", "valid"):
        d = np.load(os.path.join(HERE, f"gdb13_1K-debug_{split}.npz"))
        idx = np.nonzero(d["APDs"][:, -1] > 0)[0]
        seen = set()
        for i in idx:                                        # first of byte-identical molecules
            key = d["nodes"][i].tobytes() + d["edges"][i].tobytes()
            if key not in seen:
                seen.add(key)
                mols.append((d["nodes"][i].astype(np.int8), d["edges"][i].astype(np.int8)))
    assert len(mols) == 20, len(mols)
    rng = np.random.default_rng(20240613)
    N, seg, Fe = 13, (5, 3), 3
    mols.append(synthetic(rng, 1, N, seg, Fe, 0))
    mols.append(synthetic(rng, 2, N, seg, Fe, 0))
    mols.append(synthetic(rng, N, N, seg, Fe, 0, chain=True))
    for deg in (2, 3, 4):
        for mixed in (False, True):
            for n in (6, 9, N):
                mols.append(synthetic(rng, n, N, seg, Fe, int(rng.integers(0, 3)), last_degree=deg, mixed_last=mixed))
    while len(mols) < 140:
        n = int(rng.integers(1, N + 1))
        mols.append(synthetic(rng, n, N, seg, Fe, int(rng.integers(0, 4))))
    return mols, N, seg, Fe


def small_config(seed, count, N, seg, Fe):
    rng = np.random.default_rng(seed)
    mols = [synthetic(rng, 1, N, seg, Fe, 0), synthetic(rng, 2, N, seg, Fe, 0), synthetic(rng, N, N, seg, Fe, 3)]
    for deg in (2, 3, 4):
        mols.append(synthetic(rng, N, N, seg, Fe, 2, last_degree=deg, mixed_last=True))
    while len(mols) < count:
        n = int(rng.integers(3, N + 1))
        mols.append(synthetic(rng, n, N, seg, Fe, int(rng.integers(0, 5))))
    return mols, N, seg, Fe


# ---- recording ------------------------------------------------------------------------------------------
def record(MG, mols, N, seg, Fe):
    dim_f_add, dim_f_conn = [N] + list(seg) + [Fe], [N, Fe]
    K = namedtuple("K", "dim_f_add dim_f_conn n_edge_features max_n_nodes n_node_features")
    constants = K(dim_f_add, dim_f_conn, Fe, N, sum(seg))
    width = int(np.prod(dim_f_add)) + N * Fe + 1
    rn, re, hot, rm, rs = [], [], [], [], []
    for m, (nodes, edges) in enumerate(mols):
        g = object.__new__(MG.PreprocessingGraph)
        g.constants = constants
        g.node_features = nodes.astype(np.int32)
        g.edge_features = edges.astype(np.int32)
        g.n_nodes = int(nodes.any(axis=1).sum())
        length = g.get_decoding_route_length()
        assert length == int(edges.sum()) // 2 + 2
        for k in range(length):
            (X, E), apd = g.get_decoding_route_state(k)
            apd = np.asarray(apd)
            assert apd.shape == (width,) and apd.sum() == 1 and apd.max() == 1, (m, k)
            rn.append(np.asarray(X).astype(np.int8)); re.append(np.asarray(E).astype(np.int8))
            hot.append(int(np.argmax(apd))); rm.append(m); rs.append(k)
        assert not rn[-1].any() and not re[-1].any()         # the route ends on the empty graph
    return dict(mol_nodes=np.stack([a for a, _ in mols]), mol_edges=np.stack([b for _, b in mols]),
                dim_f_add=np.array(dim_f_add), dim_f_conn=np.array(dim_f_conn),
                rows_nodes=np.stack(rn), rows_edges=np.stack(re), hot=np.array(hot, dtype=np.int32),
                row_mol=np.array(rm, dtype=np.int32), row_step=np.array(rs, dtype=np.int32))


def main():
    warnings.simplefilter("ignore", DeprecationWarning)      # int() of a 1-element array, MolecularGraph.py:511-513
    MG, real_util = load_reference()
    print("util.get_feature_vector_indices:", "the reference's" if real_util else "stub (see the docstring)")
    configs = {"gdb13": gdb13_molecules(), "arom5": small_config(11, 20, 13, (4, 3, 4), 4),
               "chiral6": small_config(12, 12, 40, (3, 2, 3, 2), 4)}
    blob = {"configs": np.array(list(configs)), "util_is_the_references": np.array(real_util)}
    for name, (mols, N, seg, Fe) in configs.items():
        set_segments(seg, real_util)
        rec = record(MG, mols, N, seg, Fe)
        print(name, "molecules", len(mols), "rows", len(rec["hot"]))
        blob.update({f"{name}::{k}": v for k, v in rec.items()})
    out = os.path.join(HERE, "golden_routes.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
