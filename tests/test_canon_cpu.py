"""CPU: molecule identity's golden, numpy model, binding and Python boundary (graphinvent_amd.analyze.canonical /
unique / fraction_unique / SeenSet).  No device compute is issued.

The numpy model (tests/canon_model.py) is the specification the device is held to bit for bit.  Here it is pinned to
tests/golden/golden_canon.npz (tests/golden/make_golden_canon.py): isomorphism classes from networkx's VF2 matcher,
node orders under which the form must not change, and the graphs on which it is known to change."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import canon_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["gdb13", "arom5", "chiral6"]
_CACHE = {}


def golden(golden_dir):
    if "g" not in _CACHE:
        _CACHE["g"] = dict(np.load(os.path.join(golden_dir, "golden_canon.npz")))
        _CACHE["r"] = np.load(os.path.join(golden_dir, "golden_routes.npz"))
    return _CACHE["g"], _CACHE["r"]


def fixture_set(golden_dir, c):
    """(nodes, edges) of a stored set: a fixture configuration of golden_routes.npz, or sym / miss."""
    G, R = golden(golden_dir)
    if c in CONFIGS:
        return R[f"{c}::mol_nodes"], R[f"{c}::mol_edges"]
    return G[f"{c}::nodes"], G[f"{c}::edges"]


def permuted_copies(golden_dir, c, k):
    """Copy k (of 8) of every molecule of set c."""
    nodes, edges = fixture_set(golden_dir, c)
    perm = golden(golden_dir)[0][f"{c}::perm"]
    out = [CM.permute(nodes[m], edges[m], perm[m, k][perm[m, k] >= 0]) for m in range(len(nodes))]
    return np.stack([a for a, _ in out]), np.stack([b for _, b in out])


def mixed_batch(golden_dir):
    G, R = golden(golden_dir)
    nodes, edges = R["gdb13::mol_nodes"], R["gdb13::mol_edges"]
    out = [CM.permute(nodes[m], edges[m], p[p >= 0]) for m, p in zip(G["mix::src"], G["mix::perm"])]
    return np.stack([a for a, _ in out]), np.stack([b for _, b in out]), G["mix::mask"]


def model_of(golden_dir, c, k=None):
    """The model's result on set c (copy k of it), computed once and shared (read only)."""
    if (c, k) not in _CACHE:
        nodes, edges = fixture_set(golden_dir, c) if k is None else permuted_copies(golden_dir, c, k)
        _CACHE[(c, k)] = CM.canonical(nodes, edges)
    return _CACHE[(c, k)]


def test_golden_covers_what_it_should(golden_dir):
    G, R = golden(golden_dir)
    assert list(G["configs"]) == CONFIGS
    assert [R[f"{c}::mol_nodes"].shape[1] for c in CONFIGS] == [13, 13, 40] and R["arom5::mol_edges"].shape[3] == 4
    for c in CONFIGS + ["sym"]:
        nodes, _ = fixture_set(golden_dir, c)
        assert G[f"{c}::perm"].shape == (len(nodes), 8, nodes.shape[1]) and G[f"{c}::classes"].shape == (len(nodes),)
    for name in ("benzene", "cyclododecane", "cubane", "prismane", "adamantane", "decalin", "bicyclopentyl",
                 "dodecahedrane", "neopentane", "tetrahedrane", "path13", "petersen", "desargues", "moebius_kantor"):
        assert name in G["sym::names"]
    assert list(G["miss::names"]) == ["cuneane", "frucht", "shrikhande", "c6_2c3"] and (G["miss::forms"] > 1).all()
    names = list(G["sym::names"])                                      # refinement alone cannot tell these two apart
    assert G["sym::classes"][names.index("decalin")] != G["sym::classes"][names.index("bicyclopentyl")]
    B = len(G["mix::src"])
    assert G["mix::src"][0] == G["mix::src"][1] == G["mix::src"][B - 1] and 0 in G["mix::mask"]
    assert os.path.getsize(os.path.join(golden_dir, "golden_canon.npz")) < \
        os.path.getsize(os.path.join(golden_dir, "golden_reorder.npz"))


@pytest.mark.parametrize("c", CONFIGS + ["sym"])
def test_model_classes_equal_vf2_and_the_pinned_keys(golden_dir, c):
    G, _ = golden(golden_dir)
    can = model_of(golden_dir, c)
    assert not can["status"].any()
    assert np.array_equal(can["key"], G[f"{c}::key"]) and can["key"].dtype == np.uint64
    uniq, rep, counts = CM.unique(can)
    assert np.array_equal(rep, G[f"{c}::classes"])
    assert counts.tolist() == [0, len(rep), len(set(G[f"{c}::classes"].tolist()))]
    nodes, edges = fixture_set(golden_dir, c)
    for g in range(len(nodes)):                                        # order / rank / form are consistent
        n = CM.derived_n(nodes[g])
        o = can["order"][g]
        assert sorted(o[:n].tolist()) == list(range(n)) and (o[n:] == -1).all()
        assert np.array_equal(can["rank"][g][o[:n]], np.arange(n))
        assert np.array_equal(can["nodes"][g][:n], nodes[g][o[:n]]) and not can["nodes"][g][n:].any()


@pytest.mark.parametrize("c", CONFIGS + ["sym"])
def test_model_form_does_not_depend_on_the_node_order(golden_dir, c):
    base = model_of(golden_dir, c)
    for k in range(8):
        can = model_of(golden_dir, c, k)
        for name in ("key", "nodes", "edges"):
            assert np.array_equal(can[name], base[name]), (c, k, name)


def test_model_misses_split_but_never_merge(golden_dir):
    """The graphs with a refinement cell that is not an orbit come out in several forms (copies count as distinct);
    no form of theirs is the form of a different graph."""
    G, _ = golden(golden_dir)
    sym = model_of(golden_dir, "sym")
    taken = {(tuple(k.tolist()), a.tobytes(), b.tobytes()) for k, a, b in zip(sym["key"], sym["nodes"], sym["edges"])}
    forms = []
    for s in range(len(G["miss::names"])):
        mine = set()
        for k in [None] + list(range(8)):
            can = model_of(golden_dir, "miss", k)
            mine.add((tuple(can["key"][s].tolist()), can["nodes"][s].tobytes(), can["edges"][s].tobytes()))
        assert len(mine) == G["miss::forms"][s] > 1
        assert not (mine & taken) and all(not (mine & f) for f in forms)
        forms.append(mine)


def test_model_unique_mask_and_seen_set(golden_dir):
    G, _ = golden(golden_dir)
    nodes, edges, mask = mixed_batch(golden_dir)
    can = CM.canonical(nodes, edges)
    uniq, rep, counts = CM.unique(can, mask)
    assert np.array_equal(uniq, G["mix::unique"]) and np.array_equal(rep, G["mix::rep"])
    assert uniq.dtype == np.float32 and counts.tolist() == [0, int(mask.sum()), int((rep == np.arange(len(rep))).sum())]
    assert uniq[1] == 0 and uniq[-1] == 0 and uniq[5] == 1 and rep[5] == -1       # distance 1, B - 1; masked out
    seen = CM.SeenSet(64)
    new = seen.add(can, rep)
    assert np.array_equal(new != 0, rep == np.arange(len(rep))) and seen.count() == counts[2]
    assert not seen.add(can, rep).any() and seen.count() == counts[2]               # all seen now
    small = CM.SeenSet(8)
    small.add(can, rep)
    assert small.full and small.count() == 8


def test_model_status_bits():
    N, Fn, Fe = 5, 3, 2
    nodes, edges = CM.from_bonds(N, Fn, Fe, [0, 1, 2], [(0, 1, 0), (1, 2, 1)])
    nodes, edges = np.repeat(nodes[None], 7, 0), np.repeat(edges[None], 7, 0)
    nodes[1, 0, 0] = 2                                                 # a value that is not 0 / 1
    edges[2, 1, 3, 0] = edges[2, 3, 1, 0] = 1                          # a bond past n
    edges[3, 0, 2, 1] = 1                                              # one direction only
    nodes[4, 4, 1] = 1                                                 # a node row behind an empty one
    n = np.array([3, 3, 3, 3, 3, 2, 9])                                # 5: node 2 and its bond past n; 6: n > N
    can = CM.canonical(nodes, edges, n)
    assert can["status"].tolist() == [0, 8, 2, 32, 64, 64 | 2, 64]
    assert CM.canonical(nodes[:5], edges[:5])["status"].tolist() == [0, 8, 2, 32, 64]   # the derived n: the same
    for g in range(1, 7):
        assert can["order"][g].tolist() == list(range(N)) and not can["nodes"][g].any()
        assert can["key"][g].tolist() == list(CM.failed_key(g))
    uniq, rep, counts = CM.unique(can)
    assert uniq.tolist() == [1] * 7 and rep.tolist() == list(range(7)) and counts.tolist() == [8 | 2 | 32 | 64, 7, 7]


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    for name, nargs in (("gi_mol_canon", 16), ("gi_mol_unique", 14), ("gi_mol_seen_add", 9),
                        ("gi_mol_unique_ws_bytes", 1)):
        assert re.search(rf"^(int|long long)\s+{name}\s*\(", hdr, flags=re.M), name
        assert name in L.SIGNATURES and hasattr(lib, name) and len(L.SIGNATURES[name][1]) == nargs
    for name, value in (("ASYMMETRIC", 32), ("NODE_PAST_N", 64), ("COUNTS", 3)):
        assert re.search(rf"#define\s+GI_MOL_{name}\s+{value}\b", hdr) and getattr(L, "MOL_" + name) == value
    assert re.search(r"#define\s+GI_SEEN_FULL\s+1\b", hdr) and L.SEEN_FULL == 1 == CM.SEEN_FULL
    assert (CM.MOL_BOND_PAST_N, CM.MOL_VALUE, CM.MOL_ASYMMETRIC, CM.MOL_NODE_PAST_N) == \
        (L.MOL_BOND_PAST_N, L.MOL_VALUE, L.MOL_ASYMMETRIC, L.MOL_NODE_PAST_N)
    assert set(analyze.CANON_STATUS_MESSAGES) == {2, 8, 32, 64}
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # added entry points are compatible
    assert "gi_canon.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_canon.hip")).read()
    assert "getenv" not in src                                            # no new switch
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in ("gi_mol_canon", "gi_mol_unique", "gi_mol_seen_add"))
    # argument checks that need no device: nothing is launched for any of these
    canon = lambda G, N, Fn, Fe, dtype=0, nb=1: lib.gi_mol_canon(
        G, N, Fn, Fe, None, None, dtype, None, nb, None, None, None, None, None, None, None)
    assert canon(0, 13, 8, 3) == 0                                         # an empty batch: no launch
    assert canon(1, 13, 8, 3) == -1                                        # no buffers
    assert canon(0, 129, 8, 3) == -1 and canon(0, 13, 8, 9) == -1 and canon(0, 0, 8, 3) == -1
    assert canon(0, 13, 8, 3, dtype=2) == -1 and canon(0, 13, 8, 3, nb=2) == -1 and canon(0, 13, 513, 3) == -2
    assert lib.gi_mol_unique_ws_bytes(-1) == -1 and lib.gi_mol_unique_ws_bytes((1 << 29) + 1) == -2
    assert lib.gi_mol_unique_ws_bytes(0) > 0 and lib.gi_mol_unique_ws_bytes(257) >= 2 * 4 * 1024 + 4 * 257
    assert lib.gi_mol_unique(1, 13, 8, 3, *([None] * 10)) == -1            # no counts
    seen = lambda G, cap: lib.gi_mol_seen_add(G, None, None, None, None, cap, None, None, None)
    assert seen(0, 8) == 0 and seen(1, 8) == -1 and seen(0, 12) == -1 and seen(0, 0) == -1 and seen(-1, 8) == -1


def test_python_boundary_raises():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    for call in (lambda: analyze.canonical(n, e), lambda: analyze.unique(n, e), lambda: analyze.fraction_unique(n, e)):
        with pytest.raises(RuntimeError, match="no CPU"):                  # CPU tensors
            call()
    with pytest.raises(TypeError, match="tensor"):
        analyze.canonical(n.numpy(), e.numpy())
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.SeenSet(8, device="cpu")
    with pytest.raises(ValueError, match="power of two"):
        analyze.SeenSet(12, device="cuda")
    if not torch.cuda.is_available():
        return
    dn, de, dk = n.cuda(), e.cuda(), torch.zeros(2, dtype=torch.int8).cuda()   # raised before anything is launched
    seen = analyze.SeenSet(8)
    for fn in (analyze.canonical, analyze.unique, analyze.fraction_unique, seen.add):
        with pytest.raises(ValueError, match="contiguous"):
            fn(dn, de.transpose(1, 2))
        with pytest.raises(TypeError, match="float32 or both int8"):
            fn(dn.float(), de)
        with pytest.raises(ValueError, match="does not match"):
            fn(dn, de[:, :12])
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(dn, de, torch.zeros(2, dtype=torch.int8))
        with pytest.raises(TypeError, match="n_nodes"):
            fn(dn, de, dk.float())
        with pytest.raises(ValueError, match="nodes must be"):
            fn(dn[0], de)
    for fn in (analyze.unique, analyze.fraction_unique):
        with pytest.raises(RuntimeError, match="mask"):
            fn(dn, de, mask=torch.ones(2))
        with pytest.raises(ValueError, match="mask"):
            fn(dn, de, mask=torch.ones(3, device="cuda"))
