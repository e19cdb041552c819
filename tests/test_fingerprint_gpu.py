"""-m gpu: molecule scoring on the device (graphinvent_amd.analyze.fingerprint / similarity / activity /
internal_diversity: gi_mol_fingerprint, gi_fp_compare).

Every integer — bits, popcount, status, atom_id, nearest, common, union — and max_sim (one fp32 division) is compared
EXACTLY with the numpy specification tests/fingerprint_model.py, which tests/test_fingerprint_cpu.py pins to networkx's
WL classes, to hand-checked molecules and to scikit-learn's own SVC outputs.  No parity with RDKit's fingerprints is
claimed.

``decision`` is an fp32 sum; it is held to a bound DERIVED from the kernel's stated summation order (the header of
csrc/gi_fingerprint.hip): a term passes through at most k = ceil(S / 256) + 9 additions, its weight, its kernel value
and its product are rounded at most twice more (the product is fused into the addition), so with u = 2**-24
    |decision - fp64| <= (k + 2) u (|intercept| + sum_s |weight[s] K_s|)           [+ 4 u sum_s |weight[s] K_s| for RBF]
and ``proba``, the sigmoid (slope <= |prob_a| / 4) of it, to that bound times |prob_a| / 4 plus 4 u."""
import math

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import canon_model as CM
from tests import fingerprint_model as FM
from tests import rl_callers
from tests import valence_model as VM
from tests.molio import padding_intact, to_dev
from tests.test_fingerprint_cpu import SETS, fitted_svc, golden, model_fp, random_rows, set_of
from tests.test_valence_cpu import RULE_ARGS, model_rules, status_cases, stored_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.int8]
U = 2.0 ** -24
_RULES = {}


def dev_rules(name, **kw):
    if kw:
        return analyze.ValenceRules(**{**RULE_ARGS[name], **kw})
    if name not in _RULES:
        _RULES[name] = analyze.ValenceRules(**RULE_ARGS[name])
    return _RULES[name]


def run(nodes, edges, n_nodes, rules, dtype=torch.int8, misalign=1, **kw):
    n = None if n_nodes is None else torch.from_numpy(np.asarray(n_nodes)).to(DEV)
    dn, de = to_dev(nodes, dtype, misalign), to_dev(edges, dtype, misalign)
    res = analyze.fingerprint(dn, de, n, rules, atom_ids=True, **kw)
    res.host()
    assert padding_intact(dn) and padding_intact(de)
    return res


def assert_same(res, want, what=""):
    got = res.host()
    assert res.bits.is_cuda and all(getattr(res, k).dtype == torch.int32 for k in ("bits", "popcount", "status", "atom_id"))
    for name in ("bits", "popcount", "status", "atom_id"):
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])
        assert np.array_equal(getattr(res, name).cpu().numpy(), w), (what, name)    # the device views are the same


def decision_bound(model, S, kind):
    """The derived bound on |decision - fp64| (module docstring), per query row."""
    k = math.ceil(S / 256) + 9
    terms = model["abs_sum"]
    return (k + 2) * U * terms + (4 * U * terms if kind == "rbf" else 0.0)


def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ---- the fingerprint against the model ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
@pytest.mark.parametrize("c", SETS)
def test_fingerprint_equals_the_model_on_the_stored_sets(golden_dir, c, dtype):
    nodes, edges, n, r = set_of(golden_dir, c)
    want = model_fp(golden_dir, c)
    assert_same(run(nodes, edges, n, dev_rules(r), dtype=dtype), want, (c, dtype))
    assert_same(run(nodes, edges, n, dev_rules(r), dtype=dtype, misalign=0), want, (c, dtype, "aligned"))
    assert (want["popcount"] > 0).any()
    plain = analyze.fingerprint(to_dev(nodes, dtype), to_dev(edges, dtype),
                                None if n is None else torch.from_numpy(n).to(DEV), dev_rules(r))
    assert plain.atom_id is None and set(plain.host()) == {"bits", "popcount", "status"}
    assert np.array_equal(plain.host()["bits"], want["bits"])


def edge_cases():
    """name -> (nodes, edges, n_nodes or None, rules name, extra rules arguments)."""
    r = model_rules("gdb13")
    cases = {}
    carbons = [("C", 0)] * 128
    mols = [VM.molecule(128, r, carbons, [(i, (i + 1) % 128, 1 + (i % 2)) for i in range(128)]),     # a 128-cycle
            VM.molecule(128, r, [("S", 0)] + [("C", 0)] * 63 + [("N", 1)] * 64, [(0, i, 1) for i in range(1, 128)]),
            VM.molecule(128, r, [("O", 0)] * 127 + [("S", 0)], [(127, i, 2) for i in range(127)]),   # the star from 127
            VM.molecule(128, r, carbons[:127], [(i, i + 1, 1) for i in range(126)])]                 # n = 127
    cases["N_128"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {})
    mols = [VM.molecule(1, r, [("N", -1)], []), VM.molecule(1, r, [("Cl", 0)], []), VM.molecule(1, r, [], [])]
    cases["N_1"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {})
    r1 = VM.Rules(**{**RULE_ARGS["gdb13"], "bond_orders": (1,)})
    mols = [VM.molecule(9, r1, [("C", 0), ("O", 0), ("N", 0), ("C", 0)], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1)]),
            VM.molecule(9, r1, [("C", 0)] * 9, [(0, i, 1) for i in range(1, 9)])]
    cases["Fe_1"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {"bond_orders": (1,)})
    bo = (1, 2, 3, 1.5)
    r4 = VM.Rules(**{**RULE_ARGS["gdb13"], "bond_orders": bo})
    ring = [(i, (i + 1) % 6, 1.5) for i in range(6)]
    mols = [VM.molecule(13, r4, [("C", 0)] * 6, ring),                                               # benzene
            VM.molecule(13, r4, [("C", 0)] * 6, [(i, (i + 1) % 6, 1 + (i % 2)) for i in range(6)]),  # a Kekule form
            VM.molecule(13, r4, [("C", 0)] * 5 + [("N", 0), ("C", 0), ("O", 0)], ring + [(0, 6, 1), (6, 7, 3)])]
    cases["Fe_4"] = (np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]), None, "gdb13", {"bond_orders": bo})
    return cases


EDGES = edge_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
@pytest.mark.parametrize("name", list(EDGES))
def test_edge_shapes(name, dtype):
    nodes, edges, n, rname, extra = EDGES[name]
    mr = VM.Rules(**{**RULE_ARGS[rname], **extra})
    for radius, n_bits in ((2, 2048), (0, 64), (1, 4096), (4, 64), (4, 4096)):
        want = FM.fingerprint(nodes, edges, n, mr, radius=radius, n_bits=n_bits)
        assert_same(run(nodes, edges, n, dev_rules(rname, **extra), dtype=dtype, radius=radius, n_bits=n_bits), want,
                    (name, dtype, radius, n_bits))
    if name == "N_128":
        assert want["status"].tolist() == [0, 0, 0, 0] and (want["atom_id"][3, 127] == -1).all()
        assert want["popcount"][0] <= 5 and len({int(x) for x in want["ids"][1][4]}) == 3      # centre, C leaf, N+ leaf
    if name == "N_1":
        assert want["status"].tolist() == [0, 0, L.VAL_EMPTY] and want["popcount"][2] == 0
        assert 1 <= want["popcount"][0] <= 5
    if name == "Fe_4":
        assert not np.array_equal(want["bits"][0], want["bits"][1])        # no aromaticity perception


@pytest.mark.parametrize("nn", [torch.int8, torch.int32, torch.int64, None], ids=["i8", "i32", "i64", "derived"])
def test_n_nodes_of_every_width_and_batches_of_0_and_1(golden_dir, nn):
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    n = nodes.any(axis=2).sum(axis=1)
    want = model_fp(golden_dir, "gdb13")
    dn = None if nn is None else torch.from_numpy(n).to(DEV, nn)
    res = analyze.fingerprint(to_dev(nodes), to_dev(edges), dn, dev_rules("gdb13"), atom_ids=True)
    assert_same(res, want, nn)
    one = analyze.fingerprint(to_dev(nodes[27:28]), to_dev(edges[27:28]), None if dn is None else dn[27:28].clone(),
                              dev_rules("gdb13"), atom_ids=True)
    assert_same(one, {k: want[k][27:28] for k in ("bits", "popcount", "status", "atom_id")}, "one")
    none = analyze.fingerprint(to_dev(nodes[:0]), to_dev(edges[:0]), None if dn is None else dn[:0].clone(),
                               dev_rules("gdb13"), atom_ids=True)
    assert [none.host()[k].shape for k in ("bits", "popcount", "status", "atom_id")] == [(0, 64), (0,), (0,), (0, 13, 2)]
    assert len(none) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "int8"])
def test_one_molecule_per_status_bit(dtype):
    cases = status_cases()
    nodes, edges = np.stack([c[0] for c in cases.values()]), np.stack([c[1] for c in cases.values()])
    n = np.array([c[2] for c in cases.values()], np.int8)
    want = FM.fingerprint(nodes, edges, n, model_rules("gdb13"))
    assert want["status"].tolist() == [c[3] & FM.ZERO_ROW for c in cases.values()]
    res = run(nodes, edges, n, dev_rules("gdb13"), dtype=dtype)
    assert_same(res, want, dtype)
    zero = want["status"] != 0
    got = res.host()
    assert not got["bits"][zero].any() and not got["popcount"][zero].any() and (got["atom_id"][zero] == -1).all()
    assert (got["popcount"][~zero] > 0).all() and zero.sum() == len(cases) - 3


# ---- the set comparison ------------------------------------------------------------------------------------------

_SETS = {}


def compare_inputs(G, S, W):
    """Random packed rows with the special rows planted; made once per shape."""
    if (G, S, W) not in _SETS:
        rng = np.random.default_rng(1000 * G + 10 * S + W)
        q, s = random_rows(rng, G, 32 * W, 0.15), random_rows(rng, S, 32 * W, 0.2)
        s[S // 2] = 0                                                      # an all-zero set row
        if S >= 63:
            s[S - 1], s[40], s[7] = s[5], s[5], s[5]                       # duplicated set rows: the lowest wins
            q[0] = s[5]                                                    # a query equal to a set row
        else:
            q[0] = s[0] = random_rows(rng, 1, 32 * W, 0.3)[0]
        if G > 1:
            q[G - 1] = 0                                                   # an all-zero query row
        w = rng.standard_normal(S).astype(np.float32)
        _SETS[(G, S, W)] = (q, s, w)
    return _SETS[(G, S, W)]


@pytest.mark.parametrize("W", [2, 64, 128])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("G", [1, 17, 257])
def test_set_comparison(G, S, W):
    """max_sim is compared exactly: the build's fp32 division is correctly rounded."""
    q, s, w = compare_inputs(G, S, W)
    dq, ref = torch.from_numpy(q).to(DEV), analyze.FingerprintSet(s)
    sim = analyze.similarity(dq, ref)
    want = FM.compare(q, s)
    got = sim.host()
    assert sim.decision is None and set(got) == {"nearest", "common", "union", "max_sim"}
    for name in ("nearest", "common", "union", "max_sim"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, G, S, W)
    hit = 5 if S >= 63 else 0
    assert got["nearest"][0] == hit and got["max_sim"][0] == 1.0 and got["common"][0] == got["union"][0] > 0
    if G > 1:
        assert got["nearest"][G - 1] == -1 and got["max_sim"][G - 1] == 0.0
    gamma, b0, pa, pb = 2.0 / (32 * W), 0.375, -1.75, 0.125
    for kind in ("tanimoto", "rbf", "linear"):
        scale = np.float32(1.0 / (32 * W)) if kind == "linear" else np.float32(1.0)
        model = analyze.KernelModel(ref, w * scale, b0, kind, gamma=gamma, prob_a=pa, prob_b=pb)
        act = analyze.activity(dq, model)
        m = FM.compare(q, s, weight=(w * scale).astype(np.float64), kind=kind, gamma=gamma, intercept=b0, prob_a=pa,
                       prob_b=pb)
        a = act.host()
        for name in ("nearest", "common", "union", "max_sim"):
            assert np.array_equal(a[name], want[name]), (name, kind)
        bound = decision_bound(m, S, kind)
        err = np.abs(a["decision"].astype(np.float64) - m["decision"])
        print(f"{kind}: G {G} S {S} W {W}: max |decision - fp64| {err.max():.3e}, smallest bound {bound.min():.3e}, "
              f"largest err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (kind, err.max(), bound[np.argmax(err / bound)])
        perr = np.abs(a["proba"].astype(np.float64) - m["proba"])
        assert (perr <= bound * abs(pa) / 4 + 4 * U).all(), (kind, perr.max())
        if G > 1:
            assert a["proba"][G - 1] == 0.0 and m["proba"][G - 1] == 0.0
        again = analyze.activity(dq, model)                                # the same bits on every run
        assert torch.equal(act._buf, again._buf)


@pytest.mark.parametrize("kind", ["rbf", "tanimoto"])
def test_golden_svc_on_the_held_out_molecules(golden_dir, kind):
    D = golden(golden_dir)
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    rows = D["svc::test_rows"]
    fp = analyze.fingerprint(to_dev(nodes[rows]), to_dev(edges[rows]), None, dev_rules("gdb13"),
                             radius=int(D["svc::radius"]), n_bits=int(D["svc::n_bits"]))
    svc, train = fitted_svc(golden_dir, kind)
    model = analyze.KernelModel.from_sklearn(svc, analyze.FingerprintSet(train) if kind == "tanimoto" else None)
    assert model.kind == kind and len(model.support) == len(D[f"svc::{kind}::dual_coef"])
    got = analyze.activity(fp, model).host()
    f, p, gap = D[f"svc::{kind}::decision"], D[f"svc::{kind}::proba"], float(D[f"svc::{kind}::platt_gap"])
    m = FM.compare(model_fp(golden_dir, "gdb13")["bits"][rows], D[f"svc::{kind}::support"],
                   weight=D[f"svc::{kind}::dual_coef"], kind=kind, gamma=model.gamma, intercept=model.intercept,
                   prob_a=model.prob_a, prob_b=model.prob_b)
    bound = decision_bound(m, len(model.support), kind)
    assert (np.abs(got["decision"] - f) <= bound + 1e-9 * np.abs(f).max()).all()
    assert (np.abs(got["proba"] - p) <= bound * abs(model.prob_a) / 4 + 4 * U + gap).all()
    assert (np.abs(got["proba"] - m["proba"]) <= bound * abs(model.prob_a) / 4 + 4 * U).all()
    assert (got["proba"] > 0.5).any() and (got["proba"] < 0.5).any()


def test_two_runs_are_byte_identical(golden_dir):
    nodes, edges, _, _ = stored_set(golden_dir, "gdb13")
    dn, de = to_dev(nodes, torch.float32), to_dev(edges, torch.float32)
    a = analyze.fingerprint(dn, de, None, dev_rules("gdb13"), atom_ids=True)
    b = analyze.fingerprint(dn, de, None, dev_rules("gdb13"), atom_ids=True)
    assert torch.equal(a._buf, b._buf)
    ref = analyze.FingerprintSet.from_molecules(dn[:100], de[:100], None, dev_rules("gdb13"))
    assert torch.equal(ref.bits, a.bits[:100]) and len(ref) == 100 and ref.n_bits == 2048
    model = analyze.KernelModel(ref, np.linspace(-1, 1, 100), 0.1, "rbf", gamma=0.01, prob_a=-2.0, prob_b=0.0)
    x, y = analyze.activity(a, model), analyze.activity(b, model)
    assert torch.equal(x._buf, y._buf) and torch.equal(x.decision, y.decision)
    dense = analyze.FingerprintSet(FM.unpack(model_fp(golden_dir, "gdb13")["bits"][:100]))   # 0 / 1 rows, packed on the host
    assert torch.equal(dense.bits, ref.bits)


def test_host_is_one_copy_and_one_synchronisation(golden_dir, monkeypatch):
    nodes, edges, n, _ = stored_set(golden_dir, "atoms_charges")
    fp = run(nodes, edges, n, dev_rules("atoms_charges"))
    fresh = analyze.fingerprint(to_dev(nodes), to_dev(edges), torch.from_numpy(n).to(DEV), dev_rules("atoms_charges"),
                                atom_ids=True)
    model = analyze.KernelModel(analyze.FingerprintSet(fp.bits[:8].clone()), np.ones(8), 0.0)
    act = analyze.activity(fp, model)
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
    first, again = fresh.host(), fresh.host()                              # kept: nothing more is copied
    scores, scores_again = act.host(), act.host()
    monkeypatch.undo()
    assert calls == {"sync": 2, "copy": 2} and again is first and scores_again is scores
    want = model_fp(golden_dir, "atoms_charges")
    assert all(np.array_equal(first[k], want[k]) for k in ("bits", "popcount", "status", "atom_id"))
    assert set(scores) == {"nearest", "common", "union", "max_sim", "decision", "proba"}


# ---- no read-back: the RL step's score on the device -------------------------------------------------------------

def test_the_activity_score_feeds_the_rl_loss_without_a_read_back(golden_dir):
    nodes, edges, n, term = stored_set(golden_dir, "atoms_charges")
    nodes, edges = np.concatenate([nodes, nodes[:16]]), np.concatenate([edges, edges[:16]])      # planted duplicates
    n, term = np.concatenate([n, n[:16]]), np.concatenate([term, term[:16]])
    G, N = len(n), nodes.shape[1]
    dn, de, dk, dt = to_dev(nodes), to_dev(edges), torch.from_numpy(n).to(DEV), torch.from_numpy(term).to(DEV)
    g = torch.Generator().manual_seed(4)
    agent, prior = (torch.rand(G, generator=g).to(DEV) for _ in range(2))
    rules, mr, target, sigma = dev_rules("atoms_charges"), model_rules("atoms_charges"), 3, 20.0
    m_fp = FM.fingerprint(nodes, edges, n, mr, radius=2, n_bits=256)
    live = np.flatnonzero(m_fp["popcount"] > 0)
    support = m_fp["bits"][live[::3]]                                     # a model over a third of the batch's own rows
    S = len(support)
    coef = np.where(np.arange(S) % 2 == 0, 1.0, -0.75).astype(np.float32)
    kw = dict(kind="tanimoto", gamma=0.0, intercept=-0.125, prob_a=-6.0, prob_b=0.5)
    model = analyze.KernelModel(analyze.FingerprintSet(support), coef, kw["intercept"], "tanimoto", prob_a=kw["prob_a"],
                                prob_b=kw["prob_b"])

    def chain(valid, uniq, proba, n_nodes, termination):
        size = analyze.target_size_score(n_nodes, target, N)
        score = analyze.compute_score([size, proba], score_type="continuous", thresholds=[0.0, 0.0], uniqueness=uniq,
                                      validity=valid, termination=termination.float())
        return rl_callers.compute_loss_component(score, -agent, -prior, uniq, sigma), score, size

    fp = analyze.fingerprint(dn, de, dk, rules, n_bits=256)                # warm: modules loaded
    analyze.validity(dn, de, dk, rules, termination=dt), analyze.unique(dn, de, dk), analyze.activity(fp, model)
    analyze.internal_diversity(fp)
    honoured = _sync_debug_honoured()
    print(f"\ntorch.cuda.set_sync_debug_mode honoured on this build: {honoured}")
    if honoured:
        torch.cuda.set_sync_debug_mode("error")                            # any read-back or synchronisation raises
    try:
        res = analyze.validity(dn, de, dk, rules, termination=dt)
        uniq, _, _ = analyze.unique(dn, de, dk, mask=res.valid > 0)
        fp = analyze.fingerprint(dn, de, dk, rules, n_bits=256)
        act = analyze.activity(fp, model)
        loss, score, size = chain(res.valid, uniq, act.proba, dk, dt)
        diversity = analyze.internal_diversity(fp)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    # the same chain fed from the numpy models
    want = VM.validity(nodes, edges, n, mr, termination=term)
    m_uniq = CM.unique(CM.canonical(nodes, edges, n), want["valid"] != 0)[0]
    m_act = FM.compare(m_fp["bits"], support, weight=coef.astype(np.float64), **kw)
    w_valid, w_uniq = torch.from_numpy(want["valid"]).to(DEV), torch.from_numpy(m_uniq).to(DEV)
    w_proba = torch.from_numpy(m_act["proba"].astype(np.float32)).to(DEV)
    w_loss, w_score, w_size = chain(w_valid, w_uniq, w_proba, dk, dt)
    # everything integer-derived: exact
    assert torch.equal(res.valid, w_valid) and torch.equal(uniq, w_uniq) and torch.equal(size, w_size)
    assert np.array_equal(fp.bits.cpu().numpy(), m_fp["bits"]) and np.array_equal(fp.status.cpu().numpy(), m_fp["status"])
    assert np.array_equal(act.nearest.cpu().numpy(), m_act["nearest"])
    assert np.array_equal(size.cpu().numpy(), FM.target_size_score(n, target, N))
    assert torch.equal(score == 0, w_score == 0)
    # what passes through decision: the derived bound, pushed through the chain.  proba: bound |prob_a| / 4 + 4 u
    # (+ u / 2 for the model's own rounding to fp32); score = size * proba * masks: |size| times that, plus the
    # products' roundings; d = agent - (prior + sigma score) and loss = d d mask: 2 |d| delta_d + delta_d^2, with
    # delta_d = sigma delta_score plus the roundings of a sum whose terms cancel
    p_tol = decision_bound(m_act, S, "tanimoto") * abs(kw["prob_a"]) / 4 + 5 * U
    assert (np.abs(act.proba.cpu().numpy().astype(np.float64) - m_act["proba"]) <= p_tol).all()
    size64, score64 = np.abs(size.cpu().numpy().astype(np.float64)), np.abs(w_score.cpu().numpy().astype(np.float64))
    s_tol = size64 * p_tol + 4 * U * score64
    assert (np.abs((score - w_score).cpu().numpy().astype(np.float64)) <= s_tol).all()
    a64, p64 = agent.cpu().numpy().astype(np.float64), prior.cpu().numpy().astype(np.float64)
    d = np.abs(-a64 - (-p64 + sigma * w_score.cpu().numpy().astype(np.float64)))
    d_tol = sigma * s_tol + 4 * U * (a64 + p64 + sigma * score64)
    l_tol = 2 * d * d_tol + d_tol ** 2 + 4 * U * d * d
    assert (np.abs((loss - w_loss).cpu().numpy().astype(np.float64)) <= l_tol).all()
    assert torch.equal(loss == 0, w_loss == 0)
    # internal diversity: every row's sum within the bound, the G row sums added by torch in an order it does not
    # state (at worst one chain of G - 1 additions), then a handful of roundings of values <= 1
    rows = FM.compare(m_fp["bits"][live], m_fp["bits"][live], weight=np.ones(len(live)))
    T, m = float(rows["decision"].sum()), len(live)
    k = math.ceil(G / 256) + 9
    div_tol = ((k + 2) + (G - 1) + 2) * U * T / (m * (m - 1)) + 4 * U
    assert diversity.dim() == 0 and diversity.is_cuda and diversity.dtype == torch.float32
    assert abs(float(diversity) - FM.internal_diversity(m_fp["bits"])) <= div_tol
    assert 0.0 < FM.internal_diversity(m_fp["bits"]) < 1.0
    # the inputs have something to find
    proba = m_act["proba"]
    assert (proba > 0.5).any() and (0 < proba).any() and (proba[proba > 0] < 0.5).any()
    assert 0 < int((m_uniq == 0).sum()) and 0 < int((want["valid"] == 0).sum()) and (m_fp["popcount"] == 0).any()
    assert 0 < int((w_score != 0).sum()) < G and (term == 0).any()
