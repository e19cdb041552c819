"""-m gpu: substructure search on the device (graphinvent_amd.analyze.substructure / substructure_score:
gi_mol_substructure).

Every integer of every output — match, n_anchors, anchors, first, n_limited, status — is compared EXACTLY with the
Python specification tests/substructure_model.py, which tests/test_substructure_cpu.py pins to networkx's monomorphism
enumeration and to hand cases.  No parity with SMARTS or RDKit's matcher is claimed."""
import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import substructure_model as SM
from tests import valence_model as VM
from tests.molio import padding_intact, to_dev
from tests.test_kekulize_cpu import DRD2_ARGS, drd2_rules
from tests.test_substructure_cpu import (PATTERNS18, STORED_SETS, dodecahedrane, drd2_molecules, drd2_patterns,
                                         pattern_molecules, set_patterns, stack_patterns)
from tests.test_valence_cpu import RULE_ARGS, model_rules, status_cases, stored_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.int8]
NAMES = ("status", "match", "n_anchors", "n_limited", "anchors", "first")
_RULES, _CACHE = {}, {}


def dev_rules(name, **kw):
    args = DRD2_ARGS if name == "drd2" else RULE_ARGS[name]
    if kw:
        return analyze.ValenceRules(**{**args, **kw})
    if name not in _RULES:
        _RULES[name] = analyze.ValenceRules(**args)
    return _RULES[name]


def dev_set(patterns):
    return analyze.SubstructureSet(**stack_patterns(patterns))


def run(nodes, edges, n_nodes, rules, ps, dtype=torch.int8, misalign=1, **kw):
    n = None if n_nodes is None else torch.from_numpy(np.asarray(n_nodes)).to(DEV)
    dn, de = to_dev(nodes, dtype, misalign), to_dev(edges, dtype, misalign)
    res = analyze.substructure(dn, de, n, rules, ps, **kw)
    res.host()
    assert padding_intact(dn) and padding_intact(de)
    return res


def assert_same(res, want, what=""):
    got = res.host()
    assert set(got) == set(NAMES) and res.match.is_cuda
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def derived_n(nodes):
    present = nodes.any(axis=2)
    return np.where(present.all(axis=1), nodes.shape[1], np.argmin(present, axis=1)).astype(np.int32)


def set_model(golden_dir, c, given):
    """The model on stored set c with n_nodes given or derived, computed once and shared (read only)."""
    if (c, given) not in _CACHE:
        nodes, edges, n, _ = stored_set(golden_dir, c)
        n = (derived_n(nodes) if n is None else n) if given else None
        pats = list(set_patterns(c).values())
        _CACHE[(c, given)] = (nodes, edges, n, pats, SM.substructure(nodes, edges, n, model_rules(c), pats))
    return _CACHE[(c, given)]


# ---- the stored sets and the DRD2 molecules against the model ----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
@pytest.mark.parametrize("c", STORED_SETS)
def test_equals_the_model_on_the_stored_sets(golden_dir, c, dtype):
    for given in (True, False):
        nodes, edges, n, pats, want = set_model(golden_dir, c, given)
        ps = dev_set(pats)
        assert_same(run(nodes, edges, n, dev_rules(c), ps, dtype=dtype), want, (c, dtype, given))
        assert_same(run(nodes, edges, n, dev_rules(c), ps, dtype=dtype, misalign=0), want, (c, dtype, given, "aligned"))
    assert want["match"].any() and (want["first"] >= 0).any() and not want["n_limited"].any()


def drd2_case(golden_dir):
    """128 DRD2 molecules against the 18 patterns exact and the 18 relaxed (P = 36: nine rounds of the four waves)."""
    if "drd2" not in _CACHE:
        nodes, edges, n = drd2_molecules(golden_dir)
        rows = np.arange(0, 863, 6)[:128]
        nodes, edges, n = nodes[rows], edges[rows], n[rows]
        pats = drd2_patterns(False) + drd2_patterns(True)
        _CACHE["drd2"] = (nodes, edges, n, pats, SM.substructure(nodes, edges, n, drd2_rules(), pats))
    return _CACHE["drd2"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
def test_equals_the_model_on_the_drd2_molecules(golden_dir, dtype):
    nodes, edges, n, pats, want = drd2_case(golden_dir)
    ps = dev_set(pats)
    assert ps.Np_max == 12 and len(ps) == 36 and set(ps.n_atoms) == {1, 2, 3, 4, 5, 6, 9, 10, 12}     # Np differ
    for given in (n, None):
        assert_same(run(nodes, edges, given, dev_rules("drd2"), ps, dtype=dtype), want, (dtype, given is None))
        assert_same(run(nodes, edges, given, dev_rules("drd2"), ps, dtype=dtype, misalign=0), want, (dtype, "aligned"))
    assert not want["n_limited"].any() and not want["status"].any()
    assert want["match"].any(axis=0).all() and (want["match"][:, 18:] >= want["match"][:, :18]).all()
    assert (want["n_anchors"] > 64).sum() == 0 and (want["anchors"][:, :, 1] != 0).any()      # atoms past 31 do anchor


def test_from_smiles_and_from_molecules_build_the_same_table():
    rules = dev_rules("drd2")
    nodes, edges, n = pattern_molecules()
    for relax in (False, True):
        want = analyze.SubstructureSet(**stack_patterns(drd2_patterns(relax)), device=None).table
        a = analyze.SubstructureSet.from_smiles(list(PATTERNS18.values()), rules, relax_bonds=relax, aromatic="kekulize",
                                                names=list(PATTERNS18))
        b = analyze.SubstructureSet.from_molecules(torch.from_numpy(nodes).to(DEV), torch.from_numpy(edges).to(DEV),
                                                   torch.from_numpy(n).to(DEV), rules, relax_bonds=relax)
        assert np.array_equal(a.table, want) and np.array_equal(b.table, want) and a.names == list(PATTERNS18)
        assert a.table_dev.is_cuda and np.array_equal(a.table_dev.cpu().numpy(), want)
    with pytest.raises(ValueError, match="c1ccccc1"):                      # aromatic input needs aromatic="kekulize"
        analyze.SubstructureSet.from_smiles(["CC", "c1ccccc1"], rules)
    with pytest.raises(ValueError, match="C1CC"):
        analyze.SubstructureSet.from_smiles(["C1CC"], rules)


# ---- small shapes where the kernel can go wrong -------------------------------------------------------------------------

def ring_case(N, Fe=3):
    """A ring of N carbons (N = 1: an atom, N = 2: a bond) in N slots, with bond type Fe - 1 on every second bond when
    Fe > 3, under the gdb13 atom rules with Fe bond types."""
    orders = {1: (1,), 3: (1, 2, 3), 8: (1, 2, 3, 1.5, 1, 2, 3, 1.5)}[Fe]
    r = VM.Rules(**{**RULE_ARGS["gdb13"], "bond_orders": orders})
    bonds = [(i, (i + 1) % N, 1) for i in range(N if N > 2 else N - 1)]
    nodes, edges = VM.molecule(N, r, [("C", 0)] * N, bonds)
    if Fe == 8:                                              # every second bond moves to the last type
        for i, j, _ in bonds[::2]:
            edges[i, j, 0] = edges[j, i, 0] = 0
            edges[i, j, 7] = edges[j, i, 7] = 1
    return r, orders, nodes, edges


def path_pattern(r, k, **kw):
    chain = VM.molecule(max(k, 1), r, [("C", 0)] * k, [(i, i + 1, 1) for i in range(k - 1)])
    return SM.from_molecule(*chain, k, r, **kw)


@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128])
def test_rings_at_the_word_edges_and_the_fold_of_anchors_onto_lanes(N):
    r, orders, nodes, edges = ring_case(N)
    pats = [path_pattern(r, 3), path_pattern(r, 1), path_pattern(r, 2), path_pattern(r, min(N, 32), relax_bonds=True)]
    want = SM.substructure(nodes[None], edges[None], None, r, pats)
    rules = dev_rules("gdb13")
    for dtype in DTYPES:
        for P in (1, 4):
            sub = {k: (v if k == "status" else v[:, :P]) for k, v in want.items()}
            sub["first"] = sub["first"][:, :, :max(p.Np for p in pats[:P])]
            assert_same(run(nodes[None], edges[None], None, rules, dev_set(pats[:P]), dtype=dtype), sub, (N, dtype, P))
    assert want["n_anchors"][0].tolist() == [N if N >= 3 else 0, N, N if N >= 2 else 0, N]
    assert want["first"][0, 0, :3].tolist() == ([0, 1, 2] if N >= 3 else [-1] * 3)
    if N >= 3:                                               # every atom anchors: all N bits and nothing above them
        mask = sum(int(np.uint32(w)) << (32 * k) for k, w in enumerate(want["anchors"][0, 0]))
        assert mask == (1 << N) - 1


@pytest.mark.parametrize("P", [1, 4, 5, 9])
def test_pattern_counts_around_the_wave_stride(P):
    r, orders, nodes, edges = ring_case(33)
    pats = [path_pattern(r, 1 + (3 * k) % 7) for k in range(P)]         # Np 1, 4, 7, 3, 6, 2, 5, 1, 4
    mols = np.stack([nodes, nodes]), np.stack([edges, edges])
    mols[0][1, 5:] = 0                                                   # the second molecule: the path 0-1-2-3-4, n = 5
    mols[1][1, 5:] = 0
    mols[1][1, :, 5:] = 0
    want = SM.substructure(*mols, None, r, pats)
    assert want["status"].tolist() == [0, 0] and want["match"][1].tolist() == [int(p.Np <= 5) for p in pats]
    assert_same(run(*mols, None, dev_rules("gdb13"), dev_set(pats)), want, P)


@pytest.mark.parametrize("Fe", [1, L.GI_MAX_GROUPS])
def test_one_and_eight_bond_types(Fe):
    r, orders, nodes, edges = ring_case(12, Fe)
    last = np.zeros((2, 2, Fe), bool)
    last[0, 1, Fe - 1] = last[1, 0, Fe - 1] = True                        # a bond of the LAST type between any atoms
    both = last.copy()
    both[0, 1, 0] = both[1, 0, 0] = True
    A, C, _ = r.groups
    pats = [path_pattern(r, 3), path_pattern(r, 3, relax_bonds=True), SM.Pattern(np.zeros((2, A)), np.zeros((2, C)), last),
            SM.Pattern(np.zeros((2, A)), np.zeros((2, C)), both), path_pattern(r, 12, relax_bonds=True)]
    want = SM.substructure(nodes[None], edges[None], None, r, pats)
    assert want["match"][0].tolist() == [int(Fe == 1), 1, 1, 1, 1]
    for dtype in DTYPES:
        assert_same(run(nodes[None], edges[None], None, dev_rules("gdb13", bond_orders=orders), dev_set(pats), dtype=dtype),
                    want, (Fe, dtype))


def test_a_pattern_of_32_atoms_and_an_empty_batch():
    r, orders, nodes, edges = ring_case(40)
    pats = [path_pattern(r, 32), path_pattern(r, 1)]
    want = SM.substructure(nodes[None], edges[None], None, r, pats)
    assert want["match"].tolist() == [[1, 1]] and want["first"][0, 0].tolist() == list(range(32))
    ps = dev_set(pats)
    assert ps.Np_max == 32
    assert_same(run(nodes[None], edges[None], None, dev_rules("gdb13"), ps), want)
    none = analyze.substructure(to_dev(nodes[None][:0]), to_dev(edges[None][:0]), None, dev_rules("gdb13"), ps)
    assert [none.host()[k].shape for k in NAMES] == [(0,), (0, 2), (0, 2), (0, 2), (0, 2, 4), (0, 2, 32)] and len(none) == 0


# ---- status, the limit, pattern_index ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
def test_one_molecule_per_status_bit(dtype):
    cases = status_cases()
    nodes, edges = np.stack([c[0] for c in cases.values()]), np.stack([c[1] for c in cases.values()])
    n = np.array([c[2] for c in cases.values()], np.int8)
    pats = list(set_patterns("gdb13").values())
    want = SM.substructure(nodes, edges, n, model_rules("gdb13"), pats)
    assert want["status"].tolist() == [c[3] & SM.LABEL_BITS for c in cases.values()]
    bad = want["status"] != 0
    assert bad.sum() == len(cases) - 3 and not want["match"][bad].any() and (want["first"][bad] == -1).all()
    assert want["match"][~bad].any(axis=1).all()
    assert_same(run(nodes, edges, n, dev_rules("gdb13"), dev_set(pats), dtype=dtype), want, dtype)


def test_the_step_limit_on_the_device():
    nodes, edges, n, c, pattern = dodecahedrane()
    r, rules = model_rules(c), dev_rules(c)
    pats = [pattern, set_patterns(c)["CC"]]
    mols = np.stack([nodes, nodes * 0, nodes]), np.stack([edges, edges * 0, edges])
    ns = np.array([n, 0, n], np.int32)
    ps = dev_set(pats)
    for max_steps, limited in ((64, 20), (956, 20), (957, 0), (4096, 0)):
        want = SM.substructure(*mols, ns, r, pats, max_steps=max_steps)
        assert want["n_limited"][:, 0].tolist() == [limited, 0, limited] and not want["n_limited"][:, 1].any()
        assert want["status"].tolist() == [SM.SUB_STEP_LIMIT if limited else 0, VM.VAL_EMPTY] + \
            [SM.SUB_STEP_LIMIT if limited else 0]
        assert want["match"].tolist() == [[0, 1], [0, 0], [0, 1]]
        assert_same(run(*mols, ns, rules, ps, max_steps=max_steps), want, max_steps)


def test_pattern_index_pairs_equal_the_columns_of_the_full_run(golden_dir):
    nodes, edges, n, pats, want = drd2_case(golden_dir)
    G, P = len(n), len(pats)
    idx = (np.arange(G) * 5) % (P + 2) - 1                               # -1 and P are out of range
    pair = SM.substructure(nodes, edges, n, drd2_rules(), pats, pattern_index=idx)
    ok = (idx >= 0) & (idx < P)
    assert (~ok).sum() >= 4 and (pair["status"][~ok] == SM.SUB_PATTERN_INDEX).all() and not pair["match"][~ok].any()
    for name in NAMES[1:]:
        assert np.array_equal(pair[name][ok, 0], want[name][ok, idx[ok]]), name
    ps = dev_set(pats)
    res = run(nodes, edges, n, dev_rules("drd2"), ps, pattern_index=torch.from_numpy(idx.astype(np.int32)).to(DEV))
    assert_same(res, pair)
    assert res.match.shape == (G, 1) and res.first.shape == (G, 1, ps.Np_max) and res.patterns is None


def test_every_product_of_seeded_generation_contains_its_seed(golden_dir):
    from graphinvent_amd.generator import build_graphs
    from oracle import callers_oracle as CO
    from tests import seed_grow_model as SG
    from tests.test_grow_gpu import _ggnn_generator
    from tests.test_seeded_gpu import device_bank
    G, consts, model, u = _ggnn_generator(golden_dir)
    B, N, Fe = int(G["batch"]), consts.dim_f_add[0], consts.dim_f_add[-1]
    groups = list(consts.dim_f_add[1:-1])
    S = 5
    dbank = device_bank(SG.mixed_bank(N, groups, Fe, S, seed=4), consts.dim_f_add, consts.dim_f_conn)
    gen = CO.GeneratorOracle(model, B, consts, None)
    n = build_graphs(gen, consts.dim_f_add, consts.dim_f_conn, uniforms=u.to(DEV), seeds=dbank)
    symbols = ["C", "N", "O", "F", "S", "Cl", "Br", "I", "P", "Si", "Se"]
    rules = analyze.ValenceRules(symbols[:groups[0]], [0, 1, -1][:groups[1]], bond_orders=((1, 2, 3, 1.5) * 2)[:Fe],
                                 imp_H=list(range(groups[2])) if len(groups) > 2 else None)
    full = dbank.n_nodes > 0                                             # the empty seed is no pattern: out of range
    assert int(full.sum()) == S - 1 and int(dbank.n_nodes.max()) <= L.SUB_MAX_ATOMS
    ps = analyze.SubstructureSet.from_molecules(dbank.nodes[full], dbank.edges[full], dbank.n_nodes[full], rules)
    column = torch.where(full, torch.cumsum(full.int(), 0) - 1, -1).to(torch.int32)
    idx = column[gen.generated_seed[:n].long()].contiguous()
    res = analyze.substructure(gen.generated_nodes[:n].contiguous(), gen.generated_edges[:n].contiguous(),
                               gen.generated_n_nodes[:n].contiguous(), rules, ps, pattern_index=idx)
    has = idx >= 0
    assert bool(has.any()) and bool((~has).any())
    assert bool((res.match[has, 0] == 1).all()) and bool((res.status[has] == 0).all())
    assert bool((res.status[~has] == L.SUB_PATTERN_INDEX).all()) and not bool(res.match[~has].any())
    assert bool((res.n_limited == 0).all())
    got = res.host()["first"][has.cpu().numpy(), 0]
    ns = dbank.n_nodes[full][idx[has].long()].cpu().numpy()
    assert all((row[:k] >= 0).all() and (row[k:] == -1).all() for row, k in zip(got, ns))


# ---- the score, no read-back, determinism -------------------------------------------------------------------------------

def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_the_score_feeds_compute_score_without_a_read_back(golden_dir):
    nodes, edges, n, pats, want = drd2_case(golden_dir)
    names = [f"{k}{suffix}" for suffix in ("", "~") for k in PATTERNS18]
    ps = analyze.SubstructureSet(**stack_patterns(pats), names=names)
    rules = dev_rules("drd2")
    dn, de, dk = to_dev(nodes), to_dev(edges), torch.from_numpy(n).to(DEV)
    G = len(n)
    ones = torch.ones(G, device=DEV)
    size = analyze.target_size_score(dk, 30, 72)
    require, forbid = ["benzene~", 16], ["nitro", "CF3", "sulfonamide", 8, 9]
    analyze.substructure_score(analyze.substructure(dn, de, dk, rules, ps), require=require, forbid=forbid)      # warm
    honoured = _sync_debug_honoured()
    print(f"\ntorch.cuda.set_sync_debug_mode honoured on this build: {honoured}")
    if honoured:
        torch.cuda.set_sync_debug_mode("error")                            # any read-back or synchronisation raises
    try:
        res = analyze.substructure(dn, de, dk, rules, ps)
        contribution = analyze.substructure_score(res, require=require, forbid=forbid)
        score = analyze.compute_score([size, contribution], score_type="continuous", thresholds=[0.0, 0.0],
                                      uniqueness=ones, validity=ones, termination=ones)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    m = torch.from_numpy(want["match"]).to(DEV)
    col = lambda w: names.index(w) if isinstance(w, str) else w
    restated = torch.ones(G, dtype=torch.bool, device=DEV)
    for w in require:
        restated &= m[:, col(w)] == 1
    for w in forbid:
        restated &= m[:, col(w)] == 0
    assert contribution.dtype == torch.float32 and contribution.is_cuda and torch.equal(contribution, restated.float())
    assert np.array_equal(contribution.cpu().numpy(), SM.score(want["match"], [col(w) for w in require],
                                                                [col(w) for w in forbid]))
    assert torch.equal(score, size * restated.float()) and 0 < int(restated.sum()) < G
    assert_same(res, want)


def test_two_runs_are_byte_identical(golden_dir):
    nodes, edges, n, pats, _ = drd2_case(golden_dir)
    ps = dev_set(pats)
    dn, de, dk = to_dev(nodes, torch.float32), to_dev(edges, torch.float32), torch.from_numpy(n).to(DEV)
    a = analyze.substructure(dn, de, dk, dev_rules("drd2"), ps)
    b = analyze.substructure(dn, de, dk, dev_rules("drd2"), ps)
    c = analyze.substructure(dn, de, dk, dev_rules("drd2"), ps, max_steps=8)            # and with anchors given up
    d = analyze.substructure(dn, de, dk, dev_rules("drd2"), ps, max_steps=8)
    assert torch.equal(a._buf, b._buf) and torch.equal(c._buf, d._buf) and bool(c.n_limited.any())
    assert not torch.equal(a._buf, c._buf)
