"""MNN training step at the GDB-13 shape (informational; bench.py measures the flagship GGNN workload).

    python tools/bench_mnn.py [--batch 1000] [--steps 50] [--warmup 10]

Prints one JSON line: ms per step of forward + KL loss + backward + FusedAdam, forward-only ms, graphs/s, and the
CPU restatement (tests/mnn_oracle.py) forward + backward at 16 threads on a slice of the batch, per graph."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from graphinvent_amd import synthetic  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from graphinvent_amd.loss import apd_kl_loss  # noqa: E402
from graphinvent_amd.optim import FusedAdam  # noqa: E402
from tests import mnn_oracle as MO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-graphs", type=int, default=100)
    a = ap.parse_args()
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    P = MO.init_params(cfg, seed=0)
    model = mpnn.MNN(MO.as_constants(dict(cfg, device="cuda")))
    model.load_state_dict(P)
    model = model.cuda().train()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    n8, e8, a8 = synthetic.make_batch(a.batch, **sh, seed=1)
    nodes, edges, tgt = (torch.from_numpy(x).float().cuda() for x in (n8, e8, a8))

    def step():
        opt.zero_grad(set_to_none=True)
        apd_kl_loss(model(nodes, edges), tgt).backward()
        opt.step()

    def timed(fn, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / n

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    step_ms = timed(step, a.steps)
    with torch.no_grad():
        for _ in range(a.warmup):
            model(nodes, edges)
        fwd_ms = timed(lambda: model(nodes, edges), a.steps)
    torch.set_num_threads(16)
    k = min(a.cpu_graphs, a.batch)
    cn, ce, ct = (torch.from_numpy(x[:k]).float() for x in (n8, e8, a8))
    t0 = time.perf_counter()
    MO.forward_backward(P, cfg, cn, ce, ct)
    cpu_s = time.perf_counter() - t0
    print(json.dumps({"model": "MNN", "shape": "gdb13", "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
                      "step_ms": round(step_ms, 4), "forward_ms": round(fwd_ms, 4),
                      "graphs_per_s": round(a.batch / step_ms * 1e3, 1),
                      "oracle_cpu": {"threads": 16, "graphs": k, "fwd_bwd_ms_per_graph": round(cpu_s * 1e3 / k, 4)},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
