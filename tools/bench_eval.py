"""One evaluation pass of Analyzer.get_validation_likelihood on the device (informational; bench.py measures the
flagship training workload).

    python tools/bench_eval.py [--repeats 3] [--n-samples 10000,100000] [--chembl-samples 5000] [--out DIR]

Per configuration, on the same model and the same drop-in ``BlockDataLoader`` (int8 rows, prefetched counts):
  ref        the reference method's torch code, restated (tests/eval_oracle.py), on the drop-in model
  dropin     graphinvent_amd.evaluate.get_validation_likelihood
  dropin_sf  the same with ``model.sync_free = True``
Configurations: the default GGNN (h = 128, GDB-13 shape) at B = 1000 for each n_samples, and the ChEMBL-shape
AttentionGGNN at B = 250.  Synthetic rows (graphinvent_amd.synthetic), a distinct block tiled to the pass's size.
One warm-up pass per mode, then ``--repeats`` rounds that alternate the modes.  Reported: ms per pass (median,
min, max), ms per batch, passes per second, host synchronisations per pass (``set_sync_debug_mode("warn")``
warnings where this torch honours it) and ``ops.READBACKS`` per pass.  Writes DIR/bench_eval.json and prints it."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphinvent_amd import evaluate as E  # noqa: E402
from graphinvent_amd import ops, synthetic  # noqa: E402
from graphinvent_amd.BlockDatasetLoader import BlockDataLoader, HDFDataset  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402
from tests import eval_oracle as EO  # noqa: E402

MODES = ("ref", "dropin", "dropin_sf")


def make_model(shape, kind):
    sh = synthetic.SHAPES[shape]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    cls = mpnn.AttentionGGNN if kind == "AttGGNN" else mpnn.GGNN
    model = cls(O.as_constants(dict(cfg, device="cuda")))
    model.load_state_dict(O.init_params(cfg, seed=0, model=kind))
    return model.to("cuda").eval(), sh


def make_dataset(sh, rows, distinct):
    arrays = synthetic.make_batch(distinct, sh["max_n_nodes"], sh["n_atom_types"], sh["n_formal_charge"],
                                  sh["n_edge_features"], seed=1)
    reps = (rows + distinct - 1) // distinct
    return HDFDataset.from_arrays(*(np.concatenate([a] * reps)[:rows] for a in arrays))


class Analyzer:
    def __init__(self, model, loader):
        self.model, self.valid_dataloader, self.train_dataloader = model, loader, loader


def one_pass(mode, model, ds, B, c):
    loader = BlockDataLoader(dataset=ds, batch_size=B, block_size=max(10 * B, 10000), shuffle=True, n_workers=0,
                             pin_memory=True)
    model.sync_free = mode == "dropin_sf"
    rb0 = dict(ops.READBACKS)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        t0 = time.perf_counter()
        try:
            with torch.no_grad():
                if mode == "ref":
                    like, avg = EO.validation_likelihood(model, loader, c)
                else:
                    like, avg = E.get_validation_likelihood(Analyzer(model, loader), "validation", c)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        float(avg)                                                  # the caller's use of the result
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    syncs = sum("synchroniz" in str(x.message) for x in w)
    model.sync_free = False
    return ms, syncs, {k: ops.READBACKS[k] - rb0[k] for k in rb0}


def sync_debug_honoured():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device="cuda").item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


def bench(name, shape, kind, B, n_samples, repeats, distinct):
    model, sh = make_model(shape, kind)
    n_batches = n_samples // B + 1                                  # the break test: idx * B > n_samples
    ds = make_dataset(sh, (n_batches + 1) * B, distinct)
    c = namedtuple("C", "device batch_size n_samples max_n_nodes")("cuda", B, n_samples, sh["max_n_nodes"])
    res = {m: [] for m in MODES}
    info = {}
    for m in MODES:                                                 # warm-up
        one_pass(m, model, ds, B, c)
    for _ in range(repeats):
        for m in MODES:
            ms, syncs, rb = one_pass(m, model, ds, B, c)
            res[m].append(ms)
            info[m] = dict(syncs_per_pass=syncs, readbacks_per_pass=rb)
    out = dict(name=name, model=kind, shape=shape, batch=B, n_samples=n_samples, batches_per_pass=n_batches,
               apd_width=int(ds[0][2].shape[0]))
    for m in MODES:
        t = res[m]
        med = statistics.median(t)
        out[m] = dict(ms_per_pass=round(med, 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3),
                      ms_per_batch=round(med / n_batches, 4), passes_per_s=round(1e3 / med, 3), **info[m])
    out["speedup_dropin"] = round(out["ref"]["ms_per_pass"] / out["dropin"]["ms_per_pass"], 3)
    out["speedup_dropin_sf"] = round(out["ref"]["ms_per_pass"] / out["dropin_sf"]["ms_per_pass"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-samples", default="10000,100000")
    ap.add_argument("--chembl-samples", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval"))
    a = ap.parse_args()
    runs = [bench(f"gdb13_ggnn_n{n}", "gdb13", "GGNN", 1000, int(n), a.repeats, 20000)
            for n in a.n_samples.split(",") if n]
    if a.chembl_samples > 0:
        runs.append(bench(f"chembl_attggnn_n{a.chembl_samples}", "chembl", "AttGGNN", 250, a.chembl_samples,
                          a.repeats, 1000))
    blob = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__,
                sync_debug_mode_honoured=sync_debug_honoured(), runs=runs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_eval.json"), "w") as f:
        json.dump(blob, f, indent=1)
    print(json.dumps(blob))


if __name__ == "__main__":
    main()
