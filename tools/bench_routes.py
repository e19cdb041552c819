"""Row-fed against route-fed training, in one process: the headline model (BASELINE config 2, batch_size 1000) over
synthetic GDB-13-shaped whole molecules (`synthetic.make_batch(..., frac_empty=0, frac_single=0)`: a spanning tree
with parent index < child index plus ring closures, i.e. a valid BFS-like node order).

  (a) rows       the molecules expanded once, unmerged, before timing starts, served from an ArraySource through
                 BlockStreamLoader — the existing row path, the baseline
  (b) routes     RouteLoader(merge=False): the same rows made on the device from the molecules
  (c) merged     RouteLoader(merge=True): identical subgraphs of a batch merged, as the reference's preprocessing does

One warm-up epoch per mode, then `--rounds` rounds that alternate the modes; median and [min - max] of rows/s.
Also: PCIe bytes per trained row both ways, and the device time of one `routes.expand` call (all its launches, HIP
events) at batch sizes 1000, 4000 and 16000 rows with the bytes it writes.

    python tools/bench_routes.py [--molecules 6000] [--rounds 3] [--out profiles/routes/bench_routes.json]
    python tools/bench_routes.py --trace-batches 20      # only RouteLoader batches, no model: for a kernel trace
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
from graphinvent_amd import dp, routes, synthetic                 # noqa: E402
from graphinvent_amd.gnn import mpnn                              # noqa: E402
from graphinvent_amd.loader import ArraySource, BlockStreamLoader  # noqa: E402
from graphinvent_amd.loss import apd_kl_loss                      # noqa: E402
from graphinvent_amd.optim import FusedAdam                       # noqa: E402

SH = synthetic.SHAPES["gdb13"]
ADD = [SH["max_n_nodes"], SH["n_atom_types"], SH["n_formal_charge"], SH["n_edge_features"]]
CONN = [SH["max_n_nodes"], SH["n_edge_features"]]


def molecules(n, seed=0):
    parts = [synthetic.make_batch(min(2000, n - lo), **SH, seed=seed + lo, frac_empty=0.0, frac_single=0.0)
             for lo in range(0, n, 2000)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def expand_to_host(mn, me, chunk=100):
    """Every unmerged row of the molecules as int8 host arrays (chunks of <= 127 molecules keep the APDs int8)."""
    outs = [[], [], []]
    for lo in range(0, mn.shape[0], chunk):
        dn, de = (torch.from_numpy(x[lo:lo + chunk]).cuda() for x in (mn, me))
        for o, t in zip(outs, routes.expand(dn, de, ADD, CONN, merge=False)[:3]):
            o.append(t.cpu().numpy())
    return tuple(np.concatenate(o) for o in outs)


def time_expand(mn, me, rows_target, merge, reps=20):
    """Device milliseconds of one expand call (plan + rows + expand [+ merge] launches) on about rows_target rows."""
    lengths = routes.route_lengths(mn, me)
    k = int(np.searchsorted(np.cumsum(lengths), rows_target, side="right"))
    dn, de = (torch.from_numpy(x[:k]).cuda() for x in (mn, me))
    rows = int(lengths[:k].sum())
    d = routes._route_dims(k, ADD[0], dn.shape[2], ADD[-1], ADD, CONN)
    for _ in range(3):
        routes._enqueue(dn, de, d, merge, rows)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        routes._enqueue(dn, de, d, merge, rows)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    row_bytes = ADD[0] * dn.shape[2] + ADD[0] * ADD[0] * ADD[-1] + d.apd_width * (1 if k <= 127 else 4)
    ms = statistics.median(times)
    return dict(molecules=k, rows=rows, merge=merge, ms=round(ms, 4), ms_min=round(min(times), 4),
                written_bytes=rows * row_bytes, written_GBps=round(rows * row_bytes / ms / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "routes", "bench_routes.json"))
    ap.add_argument("--trace-batches", type=int, default=0)
    a = ap.parse_args()
    mn, me = molecules(a.molecules)
    lengths = routes.route_lengths(mn, me)
    if a.trace_batches:
        ld = routes.RouteLoader(mn, me, ADD, CONN, a.batch, seed=0, merge=True, prefetch_compact=False)
        for i, _ in enumerate(ld):
            if i + 1 == a.trace_batches:
                break
        torch.cuda.synchronize()
        print(f"{a.trace_batches} RouteLoader batches of <= {a.batch} rows expanded and merged")
        return
    rn, re, ra = expand_to_host(mn, me)
    assert rn.shape[0] == int(lengths.sum())
    mol_bytes, row_bytes = mn[0].nbytes + me[0].nbytes, rn[0].nbytes + re[0].nbytes + ra[0].nbytes
    print(f"{a.molecules} molecules ({mol_bytes} B each) -> {rn.shape[0]} rows ({row_bytes} B each), "
          f"{rn.shape[0] / a.molecules:.2f} rows per molecule")

    cfg, constants = bench.workload_constants("cuda")
    torch.manual_seed(0)
    model = mpnn.GGNN(constants).cuda().train()
    tr = dp.DataParallel(model, FusedAdam(model.parameters(), lr=1e-4), loss_fn=apd_kl_loss)
    loaders = {
        "rows": BlockStreamLoader(ArraySource(rn, re, ra), a.batch, block_size=10000, seed=0, device="cuda"),
        "routes": routes.RouteLoader(mn, me, ADD, CONN, a.batch, seed=0, merge=False),
        "merged": routes.RouteLoader(mn, me, ADD, CONN, a.batch, seed=0, merge=True),
    }

    def epoch(name, e):
        ld = loaders[name]
        ld.set_epoch(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = steps = 0
        for nb, eb, ab in ld:
            tr.step(nb, eb, ab)
            rows += nb.shape[0]
            steps += 1
        torch.cuda.synchronize()
        return rows, steps, time.perf_counter() - t0

    for name in loaders:                                          # warm-up
        epoch(name, 0)
    runs = {name: [] for name in loaders}
    for r in range(a.rounds):
        for name in loaders:
            runs[name].append(epoch(name, 1 + r))
    total_rows = int(lengths.sum())
    result = dict(config="BASELINE config 2 (GGNN h=128, GDB-13 shape)", batch_size=a.batch, molecules=a.molecules,
                  unmerged_rows=total_rows, rows_per_molecule=round(total_rows / a.molecules, 3), rounds=a.rounds,
                  torch=torch.__version__, device=torch.cuda.get_device_name(0), modes={})
    for name, rs in runs.items():
        rate = [rows / dt for rows, _, dt in rs]
        src_rate = [total_rows / dt for _, _, dt in rs]           # route rows consumed per second, merged or not
        result["modes"][name] = dict(
            rows_per_s=round(statistics.median(rate)), rows_per_s_min=round(min(rate)), rows_per_s_max=round(max(rate)),
            route_rows_per_s=round(statistics.median(src_rate)),
            ms_per_step=round(statistics.median(dt / steps for _, steps, dt in rs) * 1e3, 4),
            rows_per_batch=round(statistics.mean(rows / steps for rows, steps, _ in rs), 1),
            steps_per_epoch=rs[0][1],
            pcie_bytes_per_trained_row=round(row_bytes if name == "rows" else mol_bytes * a.molecules / rs[0][0], 1))
        m = result["modes"][name]
        print(f"{name:7s} {m['rows_per_s']:>9,d} rows/s [{m['rows_per_s_min']:,d} - {m['rows_per_s_max']:,d}]  "
              f"{m['ms_per_step']:.3f} ms/step  {m['rows_per_batch']:.1f} rows/batch  "
              f"{m['pcie_bytes_per_trained_row']} B over PCIe per trained row")
    b, base = result["modes"]["routes"], result["modes"]["rows"]
    result["condition"] = dict(text="(b) routes median rows/s >= (a) rows minimum rows/s",
                               met=bool(b["rows_per_s"] >= base["rows_per_s_min"]),
                               ratio_to_rows_median=round(b["rows_per_s"] / base["rows_per_s"], 4))
    print("condition:", result["condition"])
    big_n, big_e = molecules(3000, seed=10 ** 6)
    result["expand_call"] = [time_expand(big_n, big_e, rows, merge) for rows in (1000, 4000, 16000)
                             for merge in (False, True)]
    for x in result["expand_call"]:
        print("expand call:", x)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
