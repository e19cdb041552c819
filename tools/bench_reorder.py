"""What a fresh node order per molecule per epoch costs: route-fed training with RouteLoader(reorder=None) — the
baseline, the loader's behaviour without the option — against reorder="bfs" and reorder="dfs", in one process, the
headline model (BASELINE config 2, batch_size 1000) over synthetic GDB-13-shaped whole molecules, as
tools/bench_routes.py.

One warm-up epoch per mode, then `--rounds` rounds that alternate the modes; median and [min - max] of rows/s per
mode and the baseline's own spread ((max - min) / median).  The claim to check: the medians differ from the baseline's
by no more than that spread.

Also the kernel alone (one gi_route_reorder launch between HIP events, median of `--reps` after 5 warm-up launches) in
microseconds and bytes moved (molecules read + molecules written) per second, drawn ranking, at
M x N = 4096 x 13, 4096 x 40 and 1024 x 128, on random trees with ring closures and, for DFS, its two worst cases: a
chain entered at an end (the longest branch) and a star (a backward step after every node).

    python tools/bench_reorder.py [--molecules 6000] [--rounds 3] [--out profiles/routes/bench_reorder.json]
    python tools/bench_reorder.py --trace-batches 20 --reorder dfs     # only loader batches: for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

import bench                                                      # noqa: E402
from graphinvent_amd import dp, routes                            # noqa: E402
from graphinvent_amd.gnn import mpnn                              # noqa: E402
from graphinvent_amd.loss import apd_kl_loss                      # noqa: E402
from graphinvent_amd.optim import FusedAdam                       # noqa: E402
from tools.bench_routes import ADD, CONN, molecules               # noqa: E402

MODES = {"none": None, "bfs": "bfs", "dfs": "dfs"}


def shaped(kind, M, N, Fn, Fe, seed=0):
    """M molecules of N nodes each: 'tree' (random parent, N // 4 ring closures), 'chain' or 'star', all in the
    identity order; chain and star are entered at node `start` through a given ranking."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros((M, N, Fn), dtype=np.int8)
    edges = np.zeros((M, N, N, Fe), dtype=np.int8)
    nodes[:, :, 0] = 1
    m = np.arange(M)
    for i in range(1, N):
        j = {"tree": rng.integers(0, i, size=M), "chain": np.full(M, i - 1), "star": np.zeros(M, dtype=np.int64)}[kind]
        t = rng.integers(0, Fe, size=M)
        edges[m, i, j, t] = edges[m, j, i, t] = 1
    if kind == "tree":
        for _ in range(N // 4):
            i, j, t = rng.integers(0, N, size=M), rng.integers(0, N, size=M), rng.integers(0, Fe, size=M)
            ok = (i != j) & ~edges[m, i, j].any(axis=1)
            edges[m[ok], i[ok], j[ok], t[ok]] = edges[m[ok], j[ok], i[ok], t[ok]] = 1
    return nodes, edges


def time_kernel(kind, route, M, N, Fn, Fe, reps):
    mn, me = shaped(kind, M, N, Fn, Fe)
    dn, de = torch.from_numpy(mn).cuda(), torch.from_numpy(me).cuda()
    rank = None
    if kind != "tree":                                            # start at node 0: the chain's end, the star's centre
        rank = torch.arange(N, dtype=torch.int32).flip(0).repeat(M, 1).cuda()
        rank[:, 0] = 0
        rank[:, N - 1] = N - 1
    for _ in range(5):
        out = routes._enqueue_reorder(dn, de, route, rank, 0, 0, None, False)
    torch.cuda.synchronize()
    assert int(out[3].max()) == 0
    times = []
    for r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        routes._enqueue_reorder(dn, de, route, rank, 0, r, None, False)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    moved = 2 * (mn.nbytes + me.nbytes)
    us = statistics.median(times)
    return dict(kind=kind, route=route, M=M, N=N, Fn=Fn, Fe=Fe, us=round(us, 2), us_min=round(min(times), 2),
                bytes_moved=moved, GBps=round(moved / us / 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "routes", "bench_reorder.json"))
    ap.add_argument("--trace-batches", type=int, default=0)
    ap.add_argument("--reorder", default="dfs", choices=["bfs", "dfs"])
    a = ap.parse_args()
    mn, me = molecules(a.molecules)
    if a.trace_batches:
        ld = routes.RouteLoader(mn, me, ADD, CONN, a.batch, seed=0, prefetch_compact=False, reorder=a.reorder)
        for i, _ in enumerate(ld):
            if i + 1 == a.trace_batches:
                break
        torch.cuda.synchronize()
        print(f"{a.trace_batches} RouteLoader batches of <= {a.batch} rows reordered ({a.reorder}), expanded and merged")
        return
    cfg, constants = bench.workload_constants("cuda")
    torch.manual_seed(0)
    model = mpnn.GGNN(constants).cuda().train()
    tr = dp.DataParallel(model, FusedAdam(model.parameters(), lr=1e-4), loss_fn=apd_kl_loss)
    loaders = {name: routes.RouteLoader(mn, me, ADD, CONN, a.batch, seed=0, reorder=mode)
               for name, mode in MODES.items()}
    total_rows = int(loaders["none"].lengths.sum())

    def epoch(name, e):
        ld = loaders[name]
        ld.set_epoch(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for nb, eb, ab in ld:
            tr.step(nb, eb, ab)
            steps += 1
        torch.cuda.synchronize()
        return steps, time.perf_counter() - t0

    for name in loaders:                                          # warm-up
        epoch(name, 0)
    runs = {name: [] for name in loaders}
    for r in range(a.rounds):
        for name in loaders:
            runs[name].append(epoch(name, 1 + r))
    result = dict(config="BASELINE config 2 (GGNN h=128, GDB-13 shape)", batch_size=a.batch, molecules=a.molecules,
                  unmerged_rows=total_rows, rounds=a.rounds, torch=torch.__version__,
                  device=torch.cuda.get_device_name(0), modes={})
    for name, rs in runs.items():
        rate = [total_rows / dt for _, dt in rs]                  # route rows consumed per second
        result["modes"][name] = dict(route_rows_per_s=round(statistics.median(rate)), min=round(min(rate)),
                                     max=round(max(rate)),
                                     ms_per_step=round(statistics.median(dt / steps for steps, dt in rs) * 1e3, 4))
        x = result["modes"][name]
        print(f"reorder={name:5s} {x['route_rows_per_s']:>9,d} route rows/s [{x['min']:,d} - {x['max']:,d}]  "
              f"{x['ms_per_step']:.3f} ms/step")
    base = result["modes"]["none"]
    spread = (base["max"] - base["min"]) / base["route_rows_per_s"]
    result["baseline_spread"] = round(spread, 4)
    result["median_vs_baseline"] = {k: round(result["modes"][k]["route_rows_per_s"] / base["route_rows_per_s"] - 1, 4)
                                    for k in ("bfs", "dfs")}
    result["within_baseline_spread"] = {k: bool(abs(v) <= spread) for k, v in result["median_vs_baseline"].items()}
    print(f"baseline spread {spread:.2%}; medians against the baseline's: {result['median_vs_baseline']} "
          f"within the spread: {result['within_baseline_spread']}")
    result["kernel"] = []
    for M, N, Fn, Fe in ((4096, 13, 8, 3), (4096, 40, 10, 4), (1024, 128, 10, 4)):
        for kind, route in (("tree", "bfs"), ("tree", "dfs"), ("chain", "dfs"), ("star", "dfs"), ("chain", "bfs")):
            result["kernel"].append(time_kernel(kind, route, M, N, Fn, Fe, a.reps))
            print("kernel:", result["kernel"][-1])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
