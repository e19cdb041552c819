"""-m gpu: model evaluation on the device (gi_eval_nll, graphinvent_amd.evaluate).

1. The kernel against fp64 numpy: W 625 and 9769, B 1 to 4000, int8 and fp32 targets, strided logits, rows with
   all-zero and multi-hot targets, NaN and +inf logits, underflowing and tiny probabilities; compacted positions,
   untouched holes, the structure count and the overflow word exactly; two runs bit for bit.
2. get_validation_likelihood / model_scores with the drop-in GGNN and the trained weights against golden_eval.npz
   (the unmodified Analyzer on the reference's CPU model).
3. The drop-in against the restatement (tests/eval_oracle.py) on the same device logits: GGNN, AttentionGGNN, MNN,
   from a list of batches and from the drop-in BlockDataLoader.
4. No host synchronisation in the loop of a sync-free model."""
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import evaluate as E
from graphinvent_amd import ops, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import eval_oracle as EO
from tests import mnn_oracle as MO
from tests.golden import ref_callers as RC
from tests.test_eval_cpu import batches, fixture, golden, logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0


# ---- 1 ------------------------------------------------------------------------------------------------------------

def _inputs(B, W, ldo, seed):
    """Logits [B, W] inside a [B, ldo] buffer, targets [B, W] (float64 on the host) and the row kinds."""
    rng = np.random.default_rng(seed)
    buf = (rng.standard_normal((B, ldo)) * 3.0).astype(np.float32)
    o = buf[:, :W]
    t = np.zeros((B, W), np.float64)
    kind = np.array(["one"] * B, dtype=object)
    for b in range(B):
        r = b % 23
        if r == 3:
            kind[b] = "zero"                                                     # T == 0: NaN, dropped
        elif r == 5:
            kind[b] = "multi"
            t[b, rng.choice(W, 4, replace=False)] = rng.integers(1, 4, 4)
        elif r == 7:
            kind[b] = "nan"
            t[b, rng.integers(W)] = 1
            o[b, rng.integers(W)] = np.nan
        elif r == 11:
            kind[b] = "inf"
            t[b, rng.integers(W)] = 1
            o[b, rng.integers(W)] = np.inf
        elif r == 13:
            kind[b] = "under"                                                    # p < 1e-46 for every target
            j = rng.choice(W, 2, replace=False)
            t[b, j] = 1
            o[b, j] = o[b].max() - 120.0
        elif r == 17:
            kind[b] = "tiny"                                                     # p ~ 1e-26: must stay finite
            j = rng.integers(W - 1)
            t[b, j] = 1
            o[b, j] = o[b].max() - 60.0
        elif r in (1, 19):
            kind[b] = "term"
            t[b, W - 1] = 1 + (r == 19)
        else:
            t[b, rng.integers(W)] = 1
    return buf, t, kind


def _fp64(o, t):
    o = o.astype(np.float64)
    with np.errstate(all="ignore"):
        m = o.max(axis=1, keepdims=True)
        e = np.exp(o - m)
        p = e / e.sum(axis=1, keepdims=True)
        s = ((t / t.sum(axis=1, keepdims=True)) * p).sum(axis=1)
    return s, p


def _run(out, tgt, dst, start, ns, err):
    E.action_nll(out, tgt, dst, start, ns, err)
    torch.cuda.synchronize()


@pytest.mark.parametrize("W", [625, 9769])
@pytest.mark.parametrize("B", [1, 7, 1000, 4000])
@pytest.mark.parametrize("tdtype", [torch.int8, torch.float32])
def test_kernel_against_fp64(W, B, tdtype):
    ldo = W + 37
    buf, t, kind = _inputs(B, W, ldo, seed=W * 7 + B)
    s64, p64 = _fp64(buf[:, :W], t)
    keep = np.isin(kind, ["one", "multi", "under", "tiny", "term"])
    assert np.array_equal(keep, ~np.isnan(s64))
    out = torch.from_numpy(buf).to(DEV)[:, :W]
    assert out.stride(0) == ldo
    tgt = torch.from_numpy(t).to(DEV, tdtype)
    start = 5
    n_keep = int(keep.sum())
    dst = torch.full((start + n_keep + 3,), SENTINEL, device=DEV)
    ns = torch.full((1,), 1.5, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _run(out, tgt, dst, start, ns, err)
    d = dst.cpu().numpy()
    assert int(err.item()) == 0
    assert (d[:start] == SENTINEL).all() and (d[start + n_keep:] == SENTINEL).all()
    got = d[start:start + n_keep]
    k = kind[keep]
    with np.errstate(divide="ignore"):
        nll64 = -np.log(s64[keep])
    under = k == "under"
    assert all(p64[b][t[b] > 0].max() < 1e-46 for b in np.where(kind == "under")[0])
    assert all(p64[b][t[b] > 0].max() > 1e-30 for b in np.where(kind == "tiny")[0])
    assert np.isposinf(got[under]).all()
    fin = ~under
    assert np.isfinite(got[fin]).all()
    assert np.abs(got[fin] - nll64[fin]).max(initial=0) <= 1e-5 * np.abs(nll64[fin]).max(initial=1.0)
    assert (np.abs(got[fin] - nll64[fin]) <= 1e-5 * np.abs(nll64[fin]) + 1e-6).all()
    assert float(ns.item()) == 1.5 + float(t[:, -1].sum())                  # every row, NaN rows included
    # bit for bit on a second run
    dst2 = torch.full_like(dst, SENTINEL)
    ns2 = torch.full((1,), 1.5, device=DEV)
    _run(out, tgt, dst2, start, ns2, err)
    assert torch.equal(dst2, dst) and torch.equal(ns2, ns)


def test_kernel_overflow_writes_nothing_and_sticks():
    B, W = 300, 625
    buf, t, kind = _inputs(B, W, W, seed=4)
    out, tgt = torch.from_numpy(buf).to(DEV), torch.from_numpy(t).to(DEV, torch.int8)
    n_keep = int(np.isin(kind, ["one", "multi", "under", "tiny", "term"]).sum())
    for length, start, overflow in ((n_keep + 10, 10, False), (n_keep + 9, 10, True), (n_keep - 1, 0, True),
                                    (5, 10, True)):
        dst = torch.full((length,), SENTINEL, device=DEV)
        ns = torch.zeros(1, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        _run(out, tgt, dst, start, ns, err)
        assert int(err.item()) == int(overflow), (length, start)
        if overflow:
            assert (dst == SENTINEL).all() and float(ns.item()) == 0.0
            _run(out, tgt, dst, 0, ns, err)                     # sticky: a call that would fit is a no-op too
            assert (dst == SENTINEL).all() and float(ns.item()) == 0.0
    # a batch with no kept rows fits anywhere (the reference assigns an empty slice)
    t0 = torch.zeros(4, W, dtype=torch.int8, device=DEV)
    dst = torch.full((3,), SENTINEL, device=DEV)
    ns, err = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    _run(out[:4], t0, dst, 100, ns, err)
    assert int(err.item()) == 0 and (dst == SENTINEL).all()


# ---- 2 ------------------------------------------------------------------------------------------------------------

class Recorder:
    """The model under test, keeping (a clone of) every batch it saw and the logits it returned."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __call__(self, nodes, edges):
        out = self.model(nodes, edges)
        self.seen.append((nodes.clone(), edges.clone(), out.clone()))
        return out


def _golden_model():
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_generator.npz"))
    cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
    consts = RC.as_constants(RC.constants_dict("cuda", cfg, "/nonexistent", batch_size=16, epochs=1))
    model = mpnn.GGNN(constants=consts)
    model.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    return model.to(DEV).eval()


def _consts(batch_size, n_samples):
    return RC.as_constants(dict(device=DEV, batch_size=int(batch_size), n_samples=int(n_samples), max_n_nodes=13))


class _Analyzer:
    def __init__(self, model, valid, train):
        self.model, self.valid_dataloader, self.train_dataloader = model, valid, train


def _logit_slack(rec, ref_logits):
    """The existing logits bar (1e-4 of the row block's largest magnitude) holds, and how far the logits moved."""
    worst = 0.0
    for (_, _, out), ref in zip(rec.seen, ref_logits):
        d = float((out.cpu() - ref).abs().max())
        assert d <= 1e-4 * float(ref.abs().max()), d
        worst = max(worst, d)
    return worst


def _assert_nll_close(got, ref, slack):
    got, ref = got.cpu().numpy(), np.asarray(ref)
    assert np.array_equal(got != 0, ref != 0)                                 # the hole pattern
    assert (np.abs(got - ref) <= 1e-4 + 1e-4 * np.abs(ref) + 2 * slack).all(), np.abs(got - ref).max()


@pytest.mark.parametrize("case", ["valid16", "train16", "big", "overflow"])
def test_dropin_reproduces_the_golden(case):
    G, p = golden(), case + "::"
    dataset = str(G[p + "dataset"])
    c = _consts(G[p + "batch_size"], G[p + "n_samples"])
    loader = EO.ListLoader(*fixture(dataset), batches(G, p))
    rec = Recorder(_golden_model())
    a = _Analyzer(rec, loader, loader)
    if bool(G[p + "raises"]):
        with pytest.raises(RuntimeError, match="past the likelihoods buffer"):
            E.get_validation_likelihood(a, dataset, c)
        assert len(rec.seen) == len(G[p + "logit_off"]) - 1
        return
    like, avg = E.get_validation_likelihood(a, dataset, c)
    assert len(rec.seen) == len(G[p + "logit_off"]) - 1
    slack = _logit_slack(rec, logits(G, p))
    _assert_nll_close(like, G[p + "likelihoods"], slack)
    # the structure count, exactly: the same batches through the kernel
    dst = torch.zeros_like(like)
    ns, err = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for idx, (nodes, edges, tgt) in enumerate(loader):
        if idx == len(rec.seen):
            break
        E.action_nll(rec.seen[idx][2], tgt.to(DEV), dst, idx * c.batch_size, ns, err)
    assert torch.equal(dst, like) and np.array_equal(ns.cpu().numpy(), G[p + "n_structures"])
    ref_avg, ref_like = float(G[p + "avg"]), G[p + "likelihoods"].astype(np.float64)
    bound = ((1e-4 + 1e-4 * np.abs(ref_like) + 2 * slack) * (ref_like != 0)).sum() / float(ns.item())
    assert abs(float(avg) - ref_avg) <= bound + 1e-6 * abs(ref_avg)
    print(f"\n[{case}] logits moved {slack:.2e}; avg {float(avg):.6f} (reference {ref_avg:.6f})")


def test_dropin_model_scores_reproduce_the_golden():
    G = golden()
    c = _consts(G["scores::batch_size"], G["scores::n_samples"])
    rec = Recorder(_golden_model())
    a = _Analyzer(rec, EO.ListLoader(*fixture("validation"), batches(G, "scores::valid_")),
                  EO.ListLoader(*fixture("training"), batches(G, "scores::train_")))
    gen = torch.from_numpy(G["generated"]).to(DEV)
    d = E.model_scores(a, gen, c)
    assert list(d) == ["likelihood_val", "avg_likelihood_val", "likelihood_train", "avg_likelihood_train",
                       "likelihood_gen", "avg_likelihood_gen", "UC-JSD"]
    slack = _logit_slack(rec, logits(G, "scores::"))
    _assert_nll_close(d["likelihood_val"], G["scores::likelihood_val"], slack)
    _assert_nll_close(d["likelihood_train"], G["scores::likelihood_train"], slack)
    assert torch.equal(d["likelihood_gen"], gen)
    for k in ("avg_likelihood_val", "avg_likelihood_train", "avg_likelihood_gen"):
        assert abs(float(d[k]) - float(G["scores::" + k])) <= 1e-4 * abs(float(G["scores::" + k])) + 1e-5, k
    ref = float(G["scores::UC-JSD"])
    assert abs(d["UC-JSD"] - ref) <= 1e-4 * abs(ref), (d["UC-JSD"], ref)


# ---- 3 ------------------------------------------------------------------------------------------------------------

def _model(kind, seed=5):
    shape = synthetic.SHAPES["gdb13"]
    atoms, charges, N = shape["n_atom_types"], shape["n_formal_charge"], shape["max_n_nodes"]
    if kind == "MNN":
        cfg = MO.mnn_config(atoms, charges, N)
        model = mpnn.MNN(MO.as_constants(dict(cfg, device=DEV)))
        model.load_state_dict(MO.init_params(cfg, seed=seed))
    else:
        cfg = O.shaped_config(atoms, charges, N)
        cls = mpnn.AttentionGGNN if kind == "AttGGNN" else mpnn.GGNN
        model = cls(O.as_constants(dict(cfg, device=DEV)))
        model.load_state_dict(O.init_params(cfg, seed=seed, model=kind))
    return model.to(DEV).eval()


def _compare_with_restatement(rec, like, avg, c, int8):
    """The restatement on the batches and logits the drop-in saw: within 1e-6."""
    class Staged:
        def __iter__(self):
            for (nodes, edges, _), tgt in zip(rec.seen, targets):
                yield [nodes, edges, tgt]
    targets = rec.targets
    replay = EO.ReplayModel([out for _, _, out in rec.seen])
    ref, ref_avg = EO.validation_likelihood(replay, Staged(), c)
    assert replay.calls == len(rec.seen)
    assert torch.equal(like != 0, ref != 0)
    assert torch.allclose(like, ref, rtol=1e-6, atol=1e-6), float((like - ref).abs().max())
    assert abs(float(avg) - float(ref_avg)) <= 1e-6 * abs(float(ref_avg))
    assert all((t.dtype == torch.int8) == int8 for t in targets)


class TargetRecorder(Recorder):
    """Also keeps the batches' targets, taken from the loader the drop-in iterates."""

    def __init__(self, model, loader):
        super().__init__(model)
        self.targets, self.loader = [], loader

    def __iter__(self):
        for nodes, edges, tgt in self.loader:
            self.targets.append(tgt.clone())
            yield [nodes, edges, tgt]


@pytest.mark.parametrize("kind", ["GGNN", "AttGGNN", "MNN"])
def test_dropin_equals_the_restatement_from_a_list(kind):
    nodes, edges, apds = fixture("training")
    rows = np.random.default_rng(2).permutation(150)
    bl = [rows[i:i + 40] for i in range(0, 150, 40)]                          # 40, 40, 40, 30
    c = _consts(40, 100)
    rec = TargetRecorder(_model(kind), EO.ListLoader(nodes, edges, apds, bl, device=DEV))
    like, avg = E.get_validation_likelihood(_Analyzer(rec, None, rec), "training", c)
    assert len(rec.seen) == 3                                                  # 3 * 40 > 100 breaks
    _compare_with_restatement(rec, like, avg, c, int8=False)


@pytest.mark.parametrize("kind", ["GGNN", "AttGGNN", "MNN"])
def test_dropin_equals_the_restatement_from_the_block_loader(kind):
    from graphinvent_amd.BlockDatasetLoader import BlockDataLoader, HDFDataset
    arrays = [np.concatenate((a, b)) for a, b in zip(fixture("training"), fixture("validation"))]      # 250 rows
    dl = BlockDataLoader(dataset=HDFDataset.from_arrays(*arrays), batch_size=32, block_size=100, shuffle=True,
                         n_workers=0, pin_memory=True)
    c = _consts(32, 150)
    model = _model(kind)
    rec = TargetRecorder(model, dl)
    before = dict(ops.READBACKS)
    like, avg = E.get_validation_likelihood(_Analyzer(rec, rec, None), "validation", c)
    delta = {k: ops.READBACKS[k] - before[k] for k in before}
    print(f"\n[{kind}] read-backs of the pass: {delta}")
    assert len(rec.seen) == 5                                                  # 5 * 32 > 150 breaks
    if kind != "MNN":
        assert delta["prefetched"] >= 1 and delta["blocking"] == 0, delta     # the loader's prefetched counts
    _compare_with_restatement(rec, like, avg, c, int8=True)


# ---- 4 ------------------------------------------------------------------------------------------------------------

def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_sync_free_loop_has_no_host_sync():
    G = golden()
    model = _golden_model()
    model.sync_free = True
    c = _consts(16, 50)
    staged = [b for b in EO.ListLoader(*fixture("training"), batches(G, "train16::"), dtype=None, device=DEV)]
    a = _Analyzer(model, None, staged)
    E.get_validation_likelihood(a, "training", c)                             # first use allocates the sticky words
    torch.cuda.synchronize()
    strict = _sync_debug_honoured()
    print(f"\ntorch.cuda.set_sync_debug_mode honoured on this build: {strict}")
    before = dict(ops.READBACKS)
    if strict:
        torch.cuda.set_sync_debug_mode("error")
    try:
        like, avg = E.get_validation_likelihood(a, "training", c)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    delta = {k: ops.READBACKS[k] - before[k] for k in before}
    assert delta == {"prefetched": 0, "blocking": 0, "bounded": 4}, delta   # four forwards, none reads back
    model.sync_free = False
    ref, ref_avg = E.get_validation_likelihood(a, "training", c)
    assert torch.equal(like != 0, ref != 0)
    assert torch.allclose(like, ref, rtol=1e-5, atol=1e-5) and torch.allclose(avg, ref_avg, rtol=1e-5)
