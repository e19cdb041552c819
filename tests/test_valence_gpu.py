"""-m gpu: molecule validity on the device (graphinvent_amd.analyze.validity / fraction_valid: gi_mol_valence).

Every comparison is exact — valid, status, first_bad, the per-atom arrays, desc, counts — against the numpy
specification tests/valence_model.py, which tests/test_valence_cpu.py pins to textbook cases and to the SMILES strings
of the reference's shipped molecules.  No parity with RDKit is claimed.  The model's results on the stored sets are
computed once and shared."""
import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import rl_callers
from tests import valence_model as VM
from tests.molio import to_dev
from tests.test_valence_cpu import (RULE_ARGS, aromatic_and_h_cases, chemistry_table, model_of, model_rules, shipped,
                                    status_cases, stored_set)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.int8]
NAMES = ("valid", "status", "first_bad", "atom_valence", "atom_h", "desc", "counts")
_RULES = {}


def dev_rules(name, **kw):
    if kw:
        return analyze.ValenceRules(**{**RULE_ARGS[name], **kw})
    if name not in _RULES:
        _RULES[name] = analyze.ValenceRules(**RULE_ARGS[name])
    return _RULES[name]


def assert_same(res, want, what=""):
    got = res.host()
    assert res.valid.is_cuda and res.valid.dtype == torch.float32 and res.status.dtype == torch.int32
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])
        assert np.array_equal(getattr(res, name).cpu().numpy(), w), (what, name)    # the device views are the same


def run(nodes, edges, n_nodes, rules, dtype=torch.int8, misalign=1, termination=None, **kw):
    n = None if n_nodes is None else torch.from_numpy(np.asarray(n_nodes)).to(DEV)
    t = None if termination is None else torch.from_numpy(np.asarray(termination)).to(DEV)
    return analyze.validity(to_dev(nodes, dtype, misalign), to_dev(edges, dtype, misalign), n, rules, termination=t, **kw)


def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ---- device against model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
@pytest.mark.parametrize("c", ["gdb13", "arom5", "chiral6", "atoms_charges", "imp_h_chirality"])
def test_device_equals_the_model_on_the_stored_sets(golden_dir, c, dtype):
    nodes, edges, n, term = stored_set(golden_dir, c)
    want = model_of(golden_dir, c)
    assert_same(run(nodes, edges, n, dev_rules(c), dtype=dtype, termination=term), want, (c, dtype))
    aligned = run(nodes, edges, n, dev_rules(c), dtype=dtype, misalign=0, termination=term)
    assert_same(aligned, want, (c, dtype, "aligned"))
    if c == "gdb13":                                                       # hundreds of over-valent atoms
        assert (want["status"] & L.VAL_OVER != 0).sum() > 50 and want["valid"][:20].all()


def test_default_bond_orders_for_three_and_four_bond_types(golden_dir):
    for c in ("gdb13", "arom5"):
        nodes, edges, n, _ = stored_set(golden_dir, c)
        args = {k: v for k, v in RULE_ARGS[c].items() if k != "bond_orders"}
        assert_same(run(nodes, edges, n, analyze.ValenceRules(**args)), model_of(golden_dir, c), c)


@pytest.mark.parametrize("nn", [torch.int8, torch.int32, torch.int64, None], ids=["i8", "i32", "i64", "derived"])
def test_n_nodes_of_every_width(golden_dir, nn):
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    n = nodes.any(axis=2).sum(axis=1)
    res = analyze.validity(to_dev(nodes), to_dev(edges), None if nn is None else torch.from_numpy(n).to(DEV, nn),
                           dev_rules("gdb13"))
    assert_same(res, model_of(golden_dir, "gdb13"), nn)


def test_batch_sizes_0_1_and_257(golden_dir):
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    want = model_of(golden_dir, "gdb13")
    rules = dev_rules("gdb13")
    none = run(nodes[:0], edges[:0], None, rules)
    assert [none.host()[k].shape for k in NAMES] == [(0,), (0,), (0,), (0, 13), (0, 13), (0, 6), (4,)]
    assert none.host()["counts"].tolist() == [0, 0, 0, 0] and len(none) == 0
    assert [float(x) for x in analyze.fraction_valid(none)] == [0.0, 0.0, 0.0]
    one = run(nodes[27:28], edges[27:28], None, rules)
    assert_same(one, VM.validity(nodes[27:28], edges[27:28], None, model_rules("gdb13")), "one")
    big_n, big_e = np.concatenate([nodes, nodes[:117]]), np.concatenate([edges, edges[:117]])
    term = (np.arange(257) % 3 != 0).astype(np.int8)
    big = run(big_n, big_e, None, rules, termination=term)
    got = big.host()
    for name in NAMES[:-1]:
        assert np.array_equal(got[name], np.concatenate([want[name], want[name][:117]])), name
    ok = got["valid"] != 0
    assert got["counts"].tolist() == [int(ok.sum()), int(term.sum()), int((ok & (term != 0)).sum()), 257]


# ---- the edges of the limits ------------------------------------------------------------------------------------

def limit_cases():
    """name -> (nodes, edges, n_nodes or None, rules name, extra rules arguments)."""
    rng = np.random.default_rng(9)
    r = model_rules("gdb13")
    cases = {}
    # N = 128: a 128-atom chain (the most component rounds), the same chain from the far end, a ring, a molecule whose
    # only bond touches node 127, 128 loose atoms, and n = 127 with the last slot empty
    chain = [("C", 0)] * 128
    mols = [VM.molecule(128, r, chain, [(i, i + 1, 1) for i in range(127)]),
            VM.molecule(128, r, chain, [(i, i + 1, 1 + (i % 2)) for i in range(127)][::-1]),
            VM.molecule(128, r, chain, [(i, (i + 1) % 128, 1) for i in range(128)]),
            VM.molecule(128, r, chain, [(3, 127, 3)]),
            VM.molecule(128, r, [("S", 0)] * 128, []),
            VM.molecule(128, r, chain[:127], [(i, i + 1, 1) for i in range(0, 126, 2)])]
    cases["N_128"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {})
    # N = 65: a star whose centre has 64 bonds (valence clamps nowhere, the atom is over), nodes across a word seam
    mols = [VM.molecule(65, r, [("S", 0)] + [("C", 0)] * 64, [(0, i, 1) for i in range(1, 65)]),
            VM.molecule(65, r, [("C", 0)] * 65, [(i, 64 - i, 2) for i in range(32)])]
    cases["N_65"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {})
    # Fe = 8 with explicit bond orders, every type in use; a complete graph on 40 nodes of triple bonds: valence 117,
    # with double bonds added on 32 more nodes it passes the int8 clamp
    bo = (1, 2, 3, 1.5, 1, 1.5, 3, 2)
    r8 = VM.Rules(**{**RULE_ARGS["gdb13"], "bond_orders": bo})
    nodes, edges = VM.molecule(72, r8, [("C", 0)] * 12, [])
    for i in range(11):
        edges[i, i + 1, i % 8] = edges[i + 1, i, i % 8] = 1
    big_n, big_e = VM.molecule(72, r8, [("C", 0)] * 72, [])
    for i in range(40):
        for j in range(i + 1, 40):
            big_e[i, j, 6] = big_e[j, i, 6] = 1
    for j in range(40, 72):
        big_e[0, j, 7] = big_e[j, 0, 7] = 1
    cases["Fe_8"] = (np.stack([nodes, big_n]), np.stack([edges, big_e]), None, "gdb13", {"bond_orders": bo})
    # Fn wider than the rules' segments (a chirality-like tail, set or not), with n_nodes given
    nodes, edges = VM.molecule(9, r, [("C", 0), ("O", 0), ("N", 1)], [(0, 1, 1), (0, 2, 1)], Fn=70)
    nodes[:3, 8 + rng.integers(0, 62, 3)] = 1
    nodes[1, 69] = 1
    cases["Fn_70"] = (nodes[None], edges[None], np.array([3], np.int8), "gdb13", {})
    return cases


LIMITS = limit_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
@pytest.mark.parametrize("name", list(LIMITS))
def test_limits_of_the_dims(name, dtype):
    nodes, edges, n, rname, extra = LIMITS[name]
    mr = VM.Rules(**{**RULE_ARGS[rname], **extra})
    want = VM.validity(nodes, edges, n, mr)
    assert not (want["status"] & VM.MALFORMED).any(), want["status"]
    assert_same(run(nodes, edges, n, dev_rules(rname, **extra), dtype=dtype), want, (name, dtype))
    if name == "N_128":
        assert want["desc"][:, 4].tolist() == [1, 1, 1, 127, 128, 64]
        assert want["desc"][0].tolist() == [128, 2 * 128 + 2, 128 * 12011 + 258 * 1008, 127, 1, 0]
        assert want["desc"][2, 5] == 1 and want["desc"][3, 4] == 127 and want["atom_valence"][3, 127] == 3
        assert want["desc"][4].tolist() == [128, 256, 128 * (32060 + 2016), 0, 128, 0] and want["valid"].all()
        assert want["desc"][5, 0] == 127 and want["atom_h"][5, 127] == -1
    if name == "N_65":
        assert want["status"].tolist() == [L.VAL_OVER, 0 | L.VAL_FRAGMENTS] and want["atom_valence"][0, 0] == 64
    if name == "Fe_8":
        assert want["atom_valence"][1, 0] == 127 and want["atom_valence"][1, 1] == 117 and want["first_bad"][1] == 0
        assert want["status"].tolist() == [L.VAL_AROMATIC | L.VAL_OVER, L.VAL_OVER]     # orders 3 + 1.5 on one carbon


# ---- status bits ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
def test_one_molecule_per_status_bit(dtype):
    cases = status_cases()
    nodes, edges = np.stack([c[0] for c in cases.values()]), np.stack([c[1] for c in cases.values()])
    n = np.array([c[2] for c in cases.values()], np.int8)
    want = VM.validity(nodes, edges, n, model_rules("gdb13"))
    assert want["status"].tolist() == [c[3] for c in cases.values()]
    res = run(nodes, edges, n, dev_rules("gdb13"), dtype=dtype)
    assert_same(res, want, dtype)
    assert res.host()["valid"].tolist() == [float(k in ("sound", "fragments")) for k in cases]
    strict = run(nodes, edges, n, dev_rules("gdb13"), dtype=dtype, require_connected=True)          # two fragments
    assert_same(strict, VM.validity(nodes, edges, n, model_rules("gdb13"), require_connected=True), dtype)
    assert strict.host()["valid"].tolist() == [float(k == "sound") for k in cases]
    if dtype == torch.float32:                                             # a fraction, a NaN, a -0.0 (which is 0)
        dn, de = to_dev(nodes, dtype), to_dev(edges, dtype)
        dn[0, 0, 0], de[1, 1, 1, 1], dn[2, 5, 5] = 0.5, float("nan"), -0.0
        status = analyze.validity(dn, de, torch.from_numpy(n).to(DEV), dev_rules("gdb13")).host()["status"]
        assert status[0] == L.MOL_VALUE and status[1] & L.MOL_VALUE and status[2] == want["status"][2]
    nodes, edges, status, fills = aromatic_and_h_cases()                    # VAL_AROMATIC, VAL_H_MISMATCH
    res = run(nodes, edges, None, dev_rules("arom5"), dtype=dtype)
    assert_same(res, VM.validity(nodes, edges, None, model_rules("arom5")), ("arom", dtype))
    assert res.host()["status"].tolist() == status and res.host()["atom_h"][:, 0].tolist() == fills


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
def test_textbook_cases_and_the_shipped_molecules(golden_dir, dtype):
    table = chemistry_table()
    nodes, edges = np.stack([c[0] for c in table.values()]), np.stack([c[1] for c in table.values()])
    res = run(nodes, edges, None, dev_rules("chem"), dtype=dtype)
    assert_same(res, VM.validity(nodes, edges, None, model_rules("chem")), dtype)
    got = res.host()
    assert got["valid"].tolist() == [float(c[2]) for c in table.values()]
    for k, (_, _, _, fills) in enumerate(table.values()):
        assert all(got["atom_h"][k, a] == h for a, h in fills.items()), k
    nodes, edges, V = shipped(golden_dir)
    got = run(nodes, edges, None, dev_rules("gdb13"), dtype=dtype).host()
    assert got["valid"].tolist() == [1.0] * 30 and not got["status"].any() and got["counts"].tolist() == [30, 0, 0, 30]
    assert np.array_equal(got["desc"][:, 1], np.concatenate([V[f"{s}::n_h"] for s in V["splits"]]))
    assert np.array_equal(got["desc"][:, 5], np.concatenate([V[f"{s}::ring_pairs"] for s in V["splits"]]))
    assert np.array_equal(got["desc"][:, 0], np.concatenate([V[f"{s}::elements"] for s in V["splits"]]).sum(axis=1))


# ---- counts, determinism, permutation ---------------------------------------------------------------------------

def test_counts_and_fraction_valid(golden_dir):
    nodes, edges, n, term = stored_set(golden_dir, "atoms_charges")
    want = model_of(golden_dir, "atoms_charges")
    dn, de, dk = to_dev(nodes), to_dev(edges), torch.from_numpy(n).to(DEV)
    for t in (term, np.zeros_like(term), np.ones_like(term)):
        for dt in (torch.from_numpy(t).to(DEV), torch.from_numpy(t).to(DEV).float(), torch.from_numpy(t != 0).to(DEV)):
            res = analyze.validity(dn, de, dk, dev_rules("atoms_charges"), termination=dt)
            ok = want["valid"] != 0
            assert res.host()["counts"].tolist() == [int(ok.sum()), int(t.sum()), int((ok & (t != 0)).sum()), len(t)]
            model = VM.fraction_valid(want["valid"], t)
            for fr in (analyze.fraction_valid(res), analyze.fraction_valid(dn, de, dk, dev_rules("atoms_charges"),
                                                                           termination=dt)):
                assert all(f.is_cuda and f.dtype == torch.float32 and f.dim() == 0 for f in fr)
                assert [np.float32(f.item()) for f in fr] == list(model), (t.sum(), fr, model)
    assert VM.fraction_valid(want["valid"], np.zeros_like(term))[1] == 0.0            # the kept quirk
    assert 0 < want["counts"][0] < len(term)
    none = analyze.validity(dn, de, dk, dev_rules("atoms_charges"))                   # no termination: nothing terminated
    assert none.host()["counts"].tolist() == [int(want["counts"][0]), 0, 0, len(term)]


def test_two_runs_are_byte_identical_and_a_permuted_batch_permutes_the_outputs(golden_dir):
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    dn, de = to_dev(nodes, torch.float32), to_dev(edges, torch.float32)
    a, b = analyze.validity(dn, de, None, dev_rules("gdb13")), analyze.validity(dn, de, None, dev_rules("gdb13"))
    assert torch.equal(a._buf, b._buf)
    perm = np.random.default_rng(2).permutation(len(nodes))
    p = run(nodes[perm], edges[perm], None, dev_rules("gdb13"), dtype=torch.float32).host()
    for name in NAMES[:-1]:
        assert np.array_equal(p[name], a.host()[name][perm]), name
    assert np.array_equal(p["counts"], a.host()["counts"])


def test_host_is_one_copy_and_one_synchronisation(golden_dir, monkeypatch):
    nodes, edges, n, term = stored_set(golden_dir, "atoms_charges")
    res = run(nodes, edges, n, dev_rules("atoms_charges"), termination=term)
    calls = {"sync": 0, "copy": 0}
    stream_sync, copy_ = torch.cuda.Stream.synchronize, torch.Tensor.copy_

    def counted_sync(self):
        calls["sync"] += 1
        return stream_sync(self)

    def counted_copy(self, src, *a, **kw):
        calls["copy"] += int(src.is_cuda and not self.is_cuda)
        return copy_(self, src, *a, **kw)

    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted_sync)
    monkeypatch.setattr(torch.Tensor, "copy_", counted_copy)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: pytest.fail("a device-wide synchronise"))
    for bad in ("cpu", "item", "tolist"):                                 # no other way to the host is taken
        monkeypatch.setattr(torch.Tensor, bad, lambda *a, _bad=bad, **kw: pytest.fail(f"Tensor.{_bad} in host()"))
    first = res.host()
    again = res.host()                                                     # kept: nothing more is copied
    monkeypatch.undo()
    assert calls == {"sync": 1, "copy": 1} and again is first
    assert all(np.array_equal(first[k], model_of(golden_dir, "atoms_charges")[k]) for k in NAMES)


# ---- no read-back: the RL step's masks on the device ----------------------------------------------------------

def test_validity_feeds_unique_the_score_and_the_rl_loss_without_a_read_back(golden_dir):
    nodes, edges, n, term = stored_set(golden_dir, "atoms_charges")
    nodes, edges = np.concatenate([nodes, nodes[:16]]), np.concatenate([edges, edges[:16]])      # planted duplicates
    n, term = np.concatenate([n, n[:16]]), np.concatenate([term, term[:16]])
    G, N = len(n), nodes.shape[1]
    dn, de, dk, dt = to_dev(nodes), to_dev(edges), torch.from_numpy(n).to(DEV), torch.from_numpy(term).to(DEV)
    g = torch.Generator().manual_seed(4)
    agent, prior = (torch.rand(G, generator=g).to(DEV) for _ in range(2))
    rules, target, sigma = dev_rules("atoms_charges"), 3, 20.0

    def chain(valid, uniq, n_nodes, termination):
        score = torch.ones(G, device=DEV) - torch.abs(n_nodes.float() - target) / (N - target)   # target_size
        score = score * uniq * valid * termination.float()                                       # compute_score :84-91
        return rl_callers.compute_loss_component(score, -agent, -prior, uniq, sigma), score

    analyze.validity(dn, de, dk, rules, termination=dt), analyze.unique(dn, de, dk)              # warm: modules loaded
    honoured = _sync_debug_honoured()
    print(f"\ntorch.cuda.set_sync_debug_mode honoured on this build: {honoured}")
    if honoured:
        torch.cuda.set_sync_debug_mode("error")                            # any read-back or synchronisation raises
    try:
        res = analyze.validity(dn, de, dk, rules, termination=dt)
        uniq, _, _ = analyze.unique(dn, de, dk, mask=res.valid > 0)
        loss, score = chain(res.valid, uniq, dk, dt)
        fractions = analyze.fraction_valid(res)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = VM.validity(nodes, edges, n, model_rules("atoms_charges"), termination=term)
    from tests import canon_model as CM
    m_uniq = CM.unique(CM.canonical(nodes, edges, n), want["valid"] != 0)[0]
    w_loss, w_score = chain(torch.from_numpy(want["valid"]).to(DEV), torch.from_numpy(m_uniq).to(DEV), dk, dt)
    assert torch.equal(loss, w_loss) and torch.equal(score, w_score)
    assert np.array_equal(uniq.cpu().numpy(), m_uniq) and 0 < int((score != 0).sum()) < G
    assert 0 < int((m_uniq == 0).sum()) and 0 < int((want["valid"] == 0).sum())
    assert [np.float32(f.item()) for f in fractions] == list(VM.fraction_valid(want["valid"], term))
