"""Golden vectors for model evaluation, produced in the build container by the UNMODIFIED reference
``Analyzer.get_validation_likelihood`` and ``Analyzer.evaluate_model`` (Analyzer.py:39-139, 708-778), with the
reference's own ``GGNN`` on CPU loaded with the trained small-model weights of golden_generator.npz (``w::*``).

Data: the shipped fixtures gdb13_1K-debug_{train,valid} (the train file's last 21 rows have all-zero APDs, so NaN
removal and the holes it leaves are exercised).  Every batch is an explicit list of row indices fed through a plain
iterable (tests/eval_oracle.py ``ListLoader``), so that no loader's shuffle can change the golden.  The cases:

* ``valid16``   batch_size 16, n_samples 40 (not a multiple: the break fires before batch 3), batch 1 ragged (9 rows)
* ``train16``   batch_size 16, n_samples 50 over shuffled train rows (zero rows inside), batch 2 ragged (11 rows)
* ``big``       batch_size 24 > n_samples 10: one batch, then the break
* ``overflow``  batch_size 1, n_samples 1 (an 18-entry buffer), batch 1 holds 30 live rows: the reference raises
* ``scores``    ``evaluate_model`` with batch_size 16, n_samples 40 on ``valid16``'s batches and on train batches,
  the generated set being the non-zero per-action likelihoods of golden_generator.npz (what ``GraphGenerator.sample``
  returns); ``_uc_jsd`` is reached through a ``util.write_validation_scores`` stub that captures ``model_scores``

Stored per case: the batches' rows, the logits the model returned for each batch it was called on, and the
results (``likelihoods``, ``avg_final_likelihood``, ``n_structures``; for ``scores`` the whole dictionary).
``n_structures`` is not returned by the reference; it is the restatement's, which must first reproduce the
unmodified method bit for bit on the same logits.

Run from the repository root: ``python tests/golden/make_golden_eval.py``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ggnn_oracle as O                # noqa: E402
from tests import eval_oracle as EO                # noqa: E402
from tests.golden import ref_callers as RC         # noqa: E402

SCORE_KEYS = ("likelihood_val", "avg_likelihood_val", "likelihood_train", "avg_likelihood_train", "likelihood_gen",
              "avg_likelihood_gen", "UC-JSD")


def fixture(name):
    D = np.load(os.path.join(HERE, f"gdb13_1K-debug_{name}.npz"))
    return D["nodes"], D["edges"], D["APDs"]


def cases():
    """name -> (dataset, batch_size, n_samples, batches); ``scores`` -> (valid batches, train batches)."""
    perm = [int(i) for i in np.random.default_rng(13).permutation(150)]
    return {
        "valid16": ("validation", 16, 40, [range(0, 16), range(16, 25), range(25, 41), range(41, 57)]),
        "train16": ("training", 16, 50, [perm[0:16], perm[16:32], perm[32:43], perm[43:59], perm[59:75]]),
        "big": ("validation", 24, 10, [range(50, 74), range(74, 98)]),
        "overflow": ("validation", 1, 1, [range(0, 5), range(5, 35), range(35, 40)]),
        "scores": (16, 40, [range(0, 16), range(16, 25), range(25, 41), range(41, 57)],
                   [perm[60:76], perm[76:92], perm[92:106], perm[106:122]]),
    }


def consts_for(cfg, batch_size, n_samples):
    d = RC.constants_dict("cpu", cfg, "/nonexistent", batch_size=batch_size, epochs=1)
    d.update(n_samples=n_samples, sample_every=1)
    return RC.as_constants(d)


def load_reference(consts):
    RC.load("reference", consts)
    sys.modules.pop("Analyzer", None)                          # ref_callers stubs it; the real class is under test
    sys.path.insert(0, RC.REF)
    try:
        import Analyzer
        import gnn.mpnn
    finally:
        sys.path.remove(RC.REF)
    assert Analyzer.__file__.startswith(RC.REF) and gnn.mpnn.__file__.startswith(RC.REF)
    return Analyzer, gnn.mpnn, sys.modules["util"]


class Recorder:
    def __init__(self, model):
        self.model, self.logits = model, []

    def __call__(self, nodes, edges):
        out = self.model(nodes, edges)
        self.logits.append(out.detach().clone())
        return out


def main():
    assert RC.have_reference()
    G = np.load(os.path.join(HERE, "golden_generator.npz"))
    cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
    AN, mpnn, util = load_reference(consts_for(cfg, 16, 40))
    model = mpnn.GGNN(consts_for(cfg, 16, 40))
    model.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    model.eval()
    data = {"validation": fixture("valid"), "training": fixture("train")}
    gen = torch.from_numpy(G["likelihoods"])
    gen = gen[gen != 0]                                        # GraphGenerator.sample, :86-88
    blob = dict(generated=gen.numpy(), cfg_keys=G["cfg_keys"], cfg_vals=G["cfg_vals"])

    def analyzer(consts, valid_batches, train_batches):
        AN.constants = consts                                  # the module's `from parameters.constants import`
        a = AN.Analyzer.__new__(AN.Analyzer)                   # (no SummaryWriter)
        a.model = Recorder(model)
        a.valid_dataloader = EO.ListLoader(*data["validation"], valid_batches)
        a.train_dataloader = EO.ListLoader(*data["training"], train_batches)
        return a

    def put_batches(prefix, batches):
        blob[prefix + "rows"] = np.concatenate([np.asarray(list(b), np.int64) for b in batches])
        blob[prefix + "row_off"] = np.cumsum([0] + [len(b) for b in batches]).astype(np.int64)

    with torch.no_grad():
        for name, spec in cases().items():
            if name == "scores":
                continue
            dataset, bs, ns, batches = spec
            consts = consts_for(cfg, bs, ns)
            a = analyzer(consts, batches, batches)
            p = f"{name}::"
            put_batches(p, batches)
            blob[p + "dataset"], blob[p + "batch_size"], blob[p + "n_samples"] = dataset, bs, ns
            try:
                like, avg = a.get_validation_likelihood(dataset=dataset)
                raised = False
            except RuntimeError as e:
                raised = True
                print(name, "raises:", str(e).splitlines()[0])
            blob[p + "raises"] = raised
            blob[p + "logits"] = torch.cat(a.model.logits).numpy()
            blob[p + "logit_off"] = np.cumsum([0] + [len(x) for x in a.model.logits]).astype(np.int64)
            replay = EO.ReplayModel(a.model.logits)
            loader = EO.ListLoader(*data[dataset], batches)
            if raised:
                try:
                    EO.validation_likelihood(replay, loader, consts)
                    raise AssertionError(f"{name}: the restatement does not raise")
                except RuntimeError:
                    pass
                continue
            mine, mine_avg, n_struct = EO.validation_likelihood(replay, loader, consts, with_count=True)
            assert torch.equal(mine, like) and torch.equal(mine_avg, avg), name
            blob[p + "likelihoods"], blob[p + "avg"] = like.numpy(), avg.numpy()
            blob[p + "n_structures"] = n_struct.numpy()
            print(name, "batches used", len(a.model.logits), "kept", int((like != 0).sum()), "of", like.numel(),
                  "avg", float(avg), "n_structures", float(n_struct[0]))

        bs, ns, vb, tb = cases()["scores"]
        consts = consts_for(cfg, bs, ns)
        a = analyzer(consts, vb, tb)
        captured = {}
        util.get_last_epoch = lambda: "Epoch 1"
        util.write_validation_scores = lambda output_dir, epoch_key, model_scores, append: captured.update(model_scores)
        util.write_training_status = lambda score: None
        a.evaluate_model(gen)
        assert tuple(captured) == SCORE_KEYS, tuple(captured)
        assert len(a.model.logits) == 6                         # batches 0-2 of each set (3 * 16 > 40 breaks)
        lv, lt = a.model.logits[:3], a.model.logits[3:]
        mine = EO.model_scores(EO.ReplayModel(lv + lt), EO.ListLoader(*data["validation"], vb),
                               EO.ListLoader(*data["training"], tb), gen, consts)
        for k in SCORE_KEYS:
            if k == "UC-JSD":
                assert mine[k] == captured[k], (mine[k], captured[k])
            else:
                assert torch.equal(mine[k], captured[k]), k
        put_batches("scores::valid_", vb)
        put_batches("scores::train_", tb)
        blob["scores::batch_size"], blob["scores::n_samples"] = bs, ns
        blob["scores::logits"] = torch.cat(a.model.logits).numpy()
        blob["scores::logit_off"] = np.cumsum([0] + [len(x) for x in a.model.logits]).astype(np.int64)
        blob["scores::n_valid_batches"] = len(lv)
        for k in SCORE_KEYS:
            v = captured[k]
            blob["scores::" + k] = np.float64(v) if k == "UC-JSD" else v.numpy()
        print("scores: UC-JSD", captured["UC-JSD"], "avg val", float(captured["avg_likelihood_val"]),
              "avg train", float(captured["avg_likelihood_train"]))
    print("Analyzer.get_validation_likelihood / evaluate_model: restatement == unmodified, bit for bit")
    np.savez_compressed(os.path.join(HERE, "golden_eval.npz"), **blob)


if __name__ == "__main__":
    with RC.isolated():
        main()
