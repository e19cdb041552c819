"""Model evaluation without a GPU: the restatement tests/eval_oracle.py against golden_eval.npz (made by the unmodified
``Analyzer.get_validation_likelihood`` / ``evaluate_model``, tests/golden/make_golden_eval.py), against the unmodified
methods themselves where the reference checkout is visible, the UC-JSD quirks, and graphinvent_amd.evaluate refusing
CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import eval_oracle as EO
from tests.golden import ref_callers as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("valid16", "train16", "big", "overflow")
DATASET_FILE = {"validation": "valid", "training": "train"}


def golden():
    return np.load(os.path.join(GOLDEN, "golden_eval.npz"))


def fixture(dataset):
    D = np.load(os.path.join(GOLDEN, f"gdb13_1K-debug_{DATASET_FILE[dataset]}.npz"))
    return D["nodes"], D["edges"], D["APDs"]


def batches(G, prefix):
    rows, off = G[prefix + "rows"], G[prefix + "row_off"]
    return [rows[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def logits(G, prefix):
    x, off = torch.from_numpy(G[prefix + "logits"]), G[prefix + "logit_off"]
    return [x[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def consts(batch_size, n_samples, device="cpu"):
    return RC.as_constants(dict(device=device, batch_size=int(batch_size), n_samples=int(n_samples), max_n_nodes=13))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_golden_bit_for_bit(case):
    G = golden()
    p = case + "::"
    dataset = str(G[p + "dataset"])
    c = consts(G[p + "batch_size"], G[p + "n_samples"])
    loader = EO.ListLoader(*fixture(dataset), batches(G, p))
    replay = EO.ReplayModel(logits(G, p))
    if bool(G[p + "raises"]):
        with pytest.raises(RuntimeError):
            EO.validation_likelihood(replay, loader, c)
        assert replay.calls == len(G[p + "logit_off"]) - 1
        return
    like, avg, n_struct = EO.validation_likelihood(replay, loader, c, with_count=True)
    assert replay.calls == len(G[p + "logit_off"]) - 1                 # the break fired where it did
    assert np.array_equal(like.numpy(), G[p + "likelihoods"])
    assert np.array_equal(avg.numpy(), G[p + "avg"])
    assert np.array_equal(n_struct.numpy(), G[p + "n_structures"])


def test_golden_cases_cover_holes_breaks_and_nan_rows():
    G = golden()
    like = G["valid16::likelihoods"]
    # ragged batch 1 (9 rows at 16..24): a hole at 25..31 before batch 2 starts at 32
    assert (like[16:25] != 0).all() and (like[25:32] == 0).all() and (like[32:48] != 0).all() and (like[48:] == 0).all()
    rows = batches(G, "train16::")
    nan_rows = sum(int((fixture("training")[2][r].sum(1) == 0).sum()) for r in rows[:4])
    assert nan_rows > 0 and int((G["train16::likelihoods"] != 0).sum()) == sum(map(len, rows[:4])) - nan_rows
    assert int(G["big::batch_size"]) > int(G["big::n_samples"]) and len(G["big::logit_off"]) == 2


def test_restatement_reproduces_model_scores():
    G = golden()
    c = consts(G["scores::batch_size"], G["scores::n_samples"])
    gen = torch.from_numpy(G["generated"])
    d = EO.model_scores(EO.ReplayModel(logits(G, "scores::")),
                        EO.ListLoader(*fixture("validation"), batches(G, "scores::valid_")),
                        EO.ListLoader(*fixture("training"), batches(G, "scores::train_")), gen, c)
    for k, v in d.items():
        if k == "UC-JSD":
            assert v == float(G["scores::UC-JSD"])
        else:
            assert np.array_equal(v.numpy(), G["scores::" + k]), k


def test_uc_jsd_matches_the_restatement_on_unequal_lengths_and_zero_tails():
    from graphinvent_amd.evaluate import uc_jsd
    g = torch.Generator().manual_seed(3)
    v = torch.cat((torch.rand(300, generator=g) * 3, torch.zeros(200)))         # a zero-padded buffer
    t = torch.cat((torch.rand(120, generator=g) * 9, torch.zeros(480)))
    s = torch.rand(350, generator=g)
    for args in ((v, t, s), (t, v, s), (v, t, s[:90]), (v[:10], t, s)):
        a, b = uc_jsd(*args), EO.uc_jsd(*args)
        assert a == b, (a, b)
    # min_len is taken over the padded lengths: the zero tail of `t` past 350 is cut, the one before it counts
    n = 350
    vn, tn, sn = (x[:n] / x[:n].sum() for x in (v, t, s))
    m = (vn + tn + sn) / 3
    kl = torch.nn.functional.kl_div
    assert uc_jsd(v, t, s) == float((kl(vn, m) + kl(tn, m) + kl(sn, m)) / 3)
    assert uc_jsd(v, t, s) != uc_jsd(v[:300], t[:300], s[:300])


def test_evaluate_refuses_cpu_tensors():
    from graphinvent_amd import evaluate as E
    out, tgt = torch.zeros(4, 625), torch.zeros(4, 625)
    with pytest.raises(RuntimeError, match="CUDA"):
        E.action_nll(out, tgt, torch.zeros(100), 0, torch.zeros(1), torch.zeros(1, dtype=torch.int32))
    G = golden()
    a = type("A", (), {})()
    a.model = EO.ReplayModel(logits(G, "valid16::"))
    a.valid_dataloader = a.train_dataloader = EO.ListLoader(*fixture("validation"), batches(G, "valid16::"))
    with pytest.raises(RuntimeError, match="CUDA"):
        E.get_validation_likelihood(a, "validation", consts(16, 40))
    with pytest.raises(ValueError, match="Invalid dataset entered."):
        E.get_validation_likelihood(a, "test", consts(16, 40))


@pytest.mark.skipif(not RC.have_reference(), reason="reference checkout not visible")
def test_restatement_equals_the_unmodified_analyzer():
    """The unmodified methods (Analyzer.py:39-139, 708-778) and the restatement on the same stored logits."""
    G = golden()
    with RC.isolated():
        RC.load("reference", consts(16, 40))
        sys.modules.pop("Analyzer", None)
        sys.path.insert(0, RC.REF)
        try:
            import Analyzer as AN
        finally:
            sys.path.remove(RC.REF)
        assert AN.__file__.startswith(RC.REF)
        for case in CASES:
            p = case + "::"
            dataset = str(G[p + "dataset"])
            AN.constants = c = consts(G[p + "batch_size"], G[p + "n_samples"])
            a = AN.Analyzer.__new__(AN.Analyzer)
            a.model = EO.ReplayModel(logits(G, p))
            a.valid_dataloader = a.train_dataloader = EO.ListLoader(*fixture(dataset), batches(G, p))
            mine = EO.ReplayModel(logits(G, p))
            loader = EO.ListLoader(*fixture(dataset), batches(G, p))
            if bool(G[p + "raises"]):
                with pytest.raises(RuntimeError):
                    a.get_validation_likelihood(dataset=dataset)
                with pytest.raises(RuntimeError):
                    EO.validation_likelihood(mine, loader, c)
                continue
            ref = a.get_validation_likelihood(dataset=dataset)
            got = EO.validation_likelihood(mine, loader, c)
            assert all(torch.equal(x, y) for x, y in zip(ref, got)), case
        AN.constants = c = RC.as_constants(dict(consts(G["scores::batch_size"], G["scores::n_samples"])._asdict(),
                                                job_type="train", sample_every=1, job_dir="/nonexistent/"))
        a = AN.Analyzer.__new__(AN.Analyzer)
        a.model = EO.ReplayModel(logits(G, "scores::"))
        a.valid_dataloader = EO.ListLoader(*fixture("validation"), batches(G, "scores::valid_"))
        a.train_dataloader = EO.ListLoader(*fixture("training"), batches(G, "scores::train_"))
        captured = {}
        util = sys.modules["util"]
        util.get_last_epoch = lambda: "Epoch 1"
        util.write_validation_scores = lambda output_dir, epoch_key, model_scores, append: captured.update(model_scores)
        util.write_training_status = lambda score: None
        gen = torch.from_numpy(G["generated"])
        a.evaluate_model(gen)
        mine = EO.model_scores(EO.ReplayModel(logits(G, "scores::")),
                               EO.ListLoader(*fixture("validation"), batches(G, "scores::valid_")),
                               EO.ListLoader(*fixture("training"), batches(G, "scores::train_")), gen, c)
        assert list(captured) == list(mine)
        for k in mine:
            assert (mine[k] == captured[k]) if k == "UC-JSD" else torch.equal(mine[k], captured[k]), k
