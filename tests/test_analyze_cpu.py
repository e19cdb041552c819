"""CPU: the molecule read-out's golden, numpy model, binding and Python boundary (graphinvent_amd.analyze).  No device
compute is issued.

The numpy model (tests/analyze_model.py) is pinned to the unmodified reference's ``get_molecular_properties`` and
``graph_to_graph`` output (tests/golden/golden_analyze.npz, written by tests/golden/make_golden_analyze.py): every
histogram and average bit for bit, every atom / bond record, and ``analyze.records`` against the recorded
``Chem.Atom`` / ``AddAtom`` / ``AddBond`` call sequences."""
import json
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import analyze_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["generator", "imp_h_chirality", "handmade"]
PROPS = ("n_nodes_hist", "avg_n_nodes", "atom_type_hist", "formal_charge_hist", "numh_hist", "chirality_hist",
         "n_edges_hist", "avg_n_edges", "edge_feature_hist", "fraction_properly_terminated")


def load_case(golden_dir, name):
    """A case of golden_analyze.npz with its inputs (the first two cases' are in the goldens they were taken from)."""
    G = np.load(os.path.join(golden_dir, "golden_analyze.npz"))
    g = {k.split("::", 1)[1]: G[k] for k in G.files if k.startswith(name + "::")}
    if name == "generator":
        S = np.load(os.path.join(golden_dir, "golden_generator.npz"))
        g.update(nodes=S["nodes"], edges=S["edges"], n_nodes=S["n_nodes"], termination=S["terminated"])
    elif name == "imp_h_chirality":
        S = np.load(os.path.join(golden_dir, "golden_grow.npz"))
        p = name + "::"
        g.update(nodes=S[p + "generated_nodes"], edges=S[p + "generated_edges"], n_nodes=S[p + "generated_n_nodes"],
                 termination=S[p + "properly_terminated"])
    g["groups"] = [int(x) for x in g["groups"]]
    g["tables"] = json.loads(str(g["tables"]))
    g["calls"] = json.loads(str(g["calls"]))
    g["flags"] = dict(use_imp_H=bool(g["use_imp_H"]), use_chirality=bool(g["use_chirality"]),
                      n_imp_H=len(g["tables"]["imp_H"] or []), n_chirality=len(g["tables"]["chirality"] or []))
    return g


def assert_props_equal(got: dict, g: dict, what=""):
    """Bit for bit: fp32 values compared as bytes; an absent segment is a list of zeros."""
    for k in PROPS:
        want, mine = g["prop::" + k], got[k]
        if isinstance(mine, list):
            assert mine == want.tolist() and all(x == 0 for x in mine), (what, k)
            continue
        mine = np.asarray(mine)
        assert mine.dtype == np.float32 and mine.shape == want.shape, (what, k, mine.dtype, mine.shape)
        assert mine.tobytes() == want.tobytes(), (what, k, mine, want)


def test_golden_covers_what_it_should(golden_dir):
    G = np.load(os.path.join(golden_dir, "golden_analyze.npz"))
    assert list(G["names"]) == CASES
    shapes = {"generator": (96, 13, 8, 3, 2), "imp_h_chirality": (80, 6, 10, 2, 4), "handmade": (8, 13, 15, 3, 4)}
    for name in CASES:
        g = load_case(golden_dir, name)
        assert (*g["nodes"].shape, g["edges"].shape[3], len(g["groups"])) == shapes[name]
        assert all(c is not None for c in g["calls"]) and not g["status"].any()   # the reference completed everywhere
        assert bool(g["derived_equal"])
    h = load_case(golden_dir, "handmade")
    deg = h["edges"].sum(axis=(2, 3))
    n = h["n_nodes"]
    assert 0 in n and 13 in n and 1 in n                               # empty, full, single atom
    assert deg.max() > 10 and h["prop::n_edges_hist"][9] >= 2          # the clamp, and degree 0 in the LAST bin
    assert any(n[g] > 1 and not h["edges"][g].any() for g in range(8))  # several atoms, no bond
    assert np.array_equal(h["edges"], h["edges"].transpose(0, 2, 1, 3))
    assert load_case(golden_dir, "imp_h_chirality")["prop::n_edges_hist"][9] > 0
    assert os.path.getsize(os.path.join(golden_dir, "golden_analyze.npz")) < 64 * 1024


@pytest.mark.parametrize("name", CASES)
def test_model_properties_equal_the_reference_bit_for_bit(golden_dir, name):
    g = load_case(golden_dir, name)
    for cast in (np.int8, np.float32):
        got = AM.properties(g["nodes"].astype(cast), g["edges"].astype(cast), g["n_nodes"], g["groups"],
                            termination=g["termination"], **g["flags"])
        assert_props_equal(got, g, (name, cast))
    # the node mask instead of n_nodes: the same histograms where no row below n_nodes is empty
    got = AM.properties(g["nodes"], g["edges"], None, g["groups"], termination=g["termination"], **g["flags"])
    assert_props_equal(got, g, (name, "derived"))


@pytest.mark.parametrize("name", CASES)
def test_model_decode_and_records_reproduce_the_recorded_calls(golden_dir, name):
    g = load_case(golden_dir, name)
    atoms, bonds, n_bonds, status = AM.decode(g["nodes"], g["edges"], g["n_nodes"], g["groups"])
    for k, v in (("atoms", atoms), ("bonds", bonds), ("n_bonds", n_bonds), ("status", status)):
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), (name, k)
    t = g["tables"]
    mols = list(analyze.records((atoms, bonds, n_bonds, status), t["atom_types"], t["formal_charge"], t["imp_H"],
                                t["chirality"], dict(enumerate(t["bondtypes"]))))
    assert len(mols) == len(g["calls"])
    for i, (mol, calls) in enumerate(zip(mols, g["calls"])):
        assert AM.calls_of(*mol) == calls, (name, i)
    assert sum(len(m[1]) for m in mols) == int(n_bonds.sum()) > 0
    # without a bond table the bare type index comes back
    bare = list(analyze.records((atoms, bonds, n_bonds, status), t["atom_types"], t["formal_charge"], t["imp_H"],
                                t["chirality"]))
    assert all(isinstance(b[2], int) for m in bare for b in m[1])


def test_model_status_bits_and_records_of_malformed_graphs():
    N, groups = 5, [3, 2]
    nodes, edges = np.zeros((6, N, 5), np.int8), np.zeros((6, N, N, 2), np.int8)
    n = np.array([2, 2, 2, 2, 2, 2], np.int8)
    nodes[:, :2, 0] = nodes[:, :2, 3] = 1
    edges[:, 0, 1, 0] = edges[:, 1, 0, 0] = 1
    nodes[1, 1, 3] = 0                                                # 1: a segment without an entry
    edges[2, 1, 3, 1] = edges[2, 3, 1, 1] = 1                         # 2: a bond past n_nodes
    edges[3, 0, 2:5, 0] = edges[3, 1, 2:5, 1] = 1                     # 4 (and 2): 7 bonds > max_bonds 3
    nodes[4, 0, 0] = 2                                                # 8
    edges[5, 0, 1, 1] = edges[5, 1, 0, 1] = 1                         # 16
    atoms, bonds, n_bonds, status = AM.decode(nodes, edges, n, groups, max_bonds=3)
    assert status.tolist() == [0, 1, 2, 4 | 2, 8, 16]
    assert n_bonds.tolist() == [1, 1, 2, 7, 1, 2] and atoms[1, 1].tolist() == [0, -1]
    assert bonds[3].tolist() == [[0, 1, 0], [0, 2, 0], [0, 3, 0]] and bonds[0].tolist() == [[0, 1, 0], [-1] * 3, [-1] * 3]
    assert bonds[5, :2].tolist() == [[0, 1, 0], [0, 1, 1]]
    mols = list(analyze.records((atoms, bonds, n_bonds, status), "CNO", [7, 9]))
    assert mols[1] is None and mols[2] is None and mols[3] is None     # the reference ends with mol = None or raises
    assert mols[0] == ([("C", 7, None, None)] * 2, [(0, 1, 0)]) and len(mols[5][1]) == 2
    assert "KeyError" in analyze.describe_status(2) and analyze.describe_status(0) == "well-formed"
    assert set(analyze.STATUS_MESSAGES) == {1, 2, 4, 8, 16}
    with pytest.raises(ValueError, match="tables"):
        list(analyze.records((atoms, bonds, n_bonds, status), "CNO", [0, 1], imp_H=[0, 1]))


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    for name, nargs in (("gi_mol_properties", 15), ("gi_mol_decode", 17)):
        assert re.search(rf"^int\s+{name}\s*\(", hdr, flags=re.M), name
        assert name in L.SIGNATURES and hasattr(lib, name) and len(L.SIGNATURES[name][1]) == nargs
    for name, value in (("ONEHOT", 1), ("BOND_PAST_N", 2), ("OVERFLOW", 4), ("VALUE", 8), ("MULTI_BOND", 16)):
        assert re.search(rf"#define\s+GI_MOL_{name}\s+{value}\b", hdr) and getattr(L, "MOL_" + name) == value
    assert re.search(r"#define\s+GI_ANALYZE_EDGE_BINS\s+10\b", hdr) and L.ANALYZE_EDGE_BINS == 10 == AM.EDGE_BINS
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # added entry points are compatible
    assert "gi_analyze.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gi_mol_properties" in integration and "gi_mol_decode" in integration
    # argument checks that need no device: nothing is launched for any of these
    props = lambda G, N, Fn, Fe, dtype=0, nb=1, max_n=13: lib.gi_mol_properties(
        G, N, Fn, Fe, None, None, dtype, None, nb, None, 0, max_n, None, None, None)
    assert props(0, 13, 8, 3) == 0                                         # an empty batch: no launch
    assert props(1, 13, 8, 3) == -1                                        # no buffers
    assert props(0, 129, 8, 3) == -1 and props(0, 13, 8, 9) == -1          # N, Fe past the limits: GI_EINVAL
    assert props(0, 0, 8, 3) == -1 and props(0, 13, 8, 3, dtype=2) == -1 and props(0, 13, 8, 3, nb=2) == -1
    assert props(0, 13, 513, 3) == -2 and props(0, 13, 8, 3, max_n=1025) == -1
    import ctypes as C
    seg = (C.c_int * 2)(5, 3)
    dec = lambda G, N, Fn, Fe, seg=seg, n_seg=2, mb=26: lib.gi_mol_decode(
        G, N, Fn, Fe, None, None, 0, None, 1, n_seg, seg, mb, None, None, None, None, None)
    assert dec(0, 13, 8, 3) == 0 and dec(1, 13, 8, 3) == -1
    assert dec(0, 13, 9, 3) == -1                                          # the segments do not sum to Fn
    assert dec(0, 13, 8, 3, n_seg=1) == -1 and dec(0, 13, 8, 3, seg=None) == -1 and dec(0, 13, 8, 3, mb=0) == -1
    assert dec(0, 129, 8, 3) == -1 and dec(0, 13, 8, 9) == -1


def test_python_boundary_raises():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    k = torch.zeros(2, dtype=torch.int8)
    for call in (lambda: analyze.molecular_properties(n, e, k, [5, 3]), lambda: analyze.decode(n, e, k, [5, 3])):
        with pytest.raises(RuntimeError, match="no CPU"):                  # CPU tensors
            call()
    with pytest.raises(TypeError, match="tensor"):
        analyze.decode(n.numpy(), e.numpy(), k, [5, 3])
    if not torch.cuda.is_available():
        return
    dn, de, dk = n.cuda(), e.cuda(), k.cuda()                              # raised before anything is launched
    for fn in (analyze.molecular_properties, analyze.decode):
        with pytest.raises(ValueError, match="sum to Fn"):
            fn(dn, de, dk, [5, 4])
        with pytest.raises(ValueError, match="sum to Fn"):
            fn(dn, de, dk, [8])
        with pytest.raises(ValueError, match="contiguous"):
            fn(dn, de.transpose(1, 2), dk, [5, 3])
        with pytest.raises(ValueError, match="contiguous"):
            fn(dn[:, :, ::2], de, dk, [2, 2])
        with pytest.raises(TypeError, match="float32 or both int8"):
            fn(dn.float(), de, dk, [5, 3])
        with pytest.raises(ValueError, match="does not match"):
            fn(dn, de[:, :12], dk, [5, 3])
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(dn, de, k, [5, 3])
        with pytest.raises(TypeError, match="n_nodes"):
            fn(dn, de, dk.float(), [5, 3])
    with pytest.raises(ValueError, match="required"):
        analyze.decode(dn, de, None, [5, 3])
    with pytest.raises(ValueError, match="max_bonds"):
        analyze.decode(dn, de, dk, [5, 3], max_bonds=0)
    with pytest.raises(ValueError, match="termination"):
        analyze.molecular_properties(dn, de, dk, [5, 3], termination=torch.zeros(3, device="cuda"))
