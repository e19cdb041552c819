"""Molecule log-likelihoods (`graphinvent_amd.likelihood`) against their torch restatement, in one process.

Per shape (GDB-13 with the headline model, BASELINE config 2; ChEMBL, W = 9769, where the APD rows the likelihood
path never writes are largest) synthetic whole molecules (`synthetic.make_batch(..., frac_empty=0, frac_single=0)`: a
valid BFS-like node order) are scored under `torch.no_grad` with `model.sync_free = True`, `batch_rows` 1000 and
`n_rows` from the host copies, two ways that alternate for `--rounds` rounds after a warm-up each:

  (a) kernels      likelihood.molecule_log_likelihood: expansion without APD rows, gi_row_loglik, gi_mol_loglik_sum
  (b) restatement  routes.expand(merge=False) WITH its APD rows, then per chunk of 1000 rows the model,
                   log_softmax, gather at the APD's argmax, index_add_ into the molecules

Printed and stored: ms per 1000 molecules (median [min - max]) and rows per molecule for both, and the device time
(HIP events) of the row kernels alone on [rows, W] logits with the bytes they read and write, as GB/s.  Numbers are
written down, nothing is asserted.

    python tools/bench_likelihood.py [--rounds 5] [--out profiles/likelihood/bench_likelihood.json]
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
from graphinvent_amd import likelihood as LL                      # noqa: E402
from graphinvent_amd import routes, synthetic                     # noqa: E402
from graphinvent_amd.gnn import mpnn                              # noqa: E402

MOLECULES = {"gdb13": 1000, "chembl": 200}
BATCH_ROWS = 1000


def molecules(shape, n, seed=0):
    sh = synthetic.SHAPES[shape]
    parts = [synthetic.make_batch(min(500, n - lo), **sh, seed=seed + lo, frac_empty=0.0, frac_single=0.0)
             for lo in range(0, n, 500)]
    add = [sh["max_n_nodes"], sh["n_atom_types"], sh["n_formal_charge"], sh["n_edge_features"]]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), add, [add[0], add[-1]]


def restatement(model, dn, de, add, conn, n_rows):
    nodes, edges, apds, row_mol, _ = routes.expand(dn, de, add, conn, merge=False, n_rows=n_rows)
    out = torch.zeros(dn.shape[0], device=dn.device)
    for a in range(0, n_rows, BATCH_ROWS):
        b = min(a + BATCH_ROWS, n_rows)
        lp = torch.log_softmax(model(nodes[a:b], edges[a:b]), dim=1)
        hot = apds[a:b].argmax(dim=1, keepdim=True)
        out.index_add_(0, row_mol[a:b].long(), lp.gather(1, hot)[:, 0])
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def row_kernels(rows, W, reps=20):
    """Device ms of gi_row_loglik and gi_row_loglik_bwd alone on [rows, W] logits."""
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(rows, W, device="cuda", generator=g) * 3
    hot = torch.randint(0, W, (rows,), device="cuda", generator=g, dtype=torch.int32)
    gr = torch.ones(rows, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {}
    _, lse = LL._row_forward(z, hot, err)
    for name, fn, nbytes in (("forward", lambda: LL._row_forward(z, hot, err), rows * W * 4),
                             ("backward", lambda: LL._row_backward(z, hot, lse, gr, err), 2 * rows * W * 4)):
        for _ in range(3):
            fn()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        ms = statistics.median(times)
        res[name] = dict(ms=round(ms, 4), ms_min=round(min(times), 4), bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1))
    return dict(rows=rows, W=W, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "likelihood", "bench_likelihood.json"))
    a = ap.parse_args()
    result = dict(torch=torch.__version__, device=torch.cuda.get_device_name(0), batch_rows=BATCH_ROWS,
                  rounds=a.rounds, shapes={}, row_kernels=[])
    for shape, n in MOLECULES.items():
        mn, me, add, conn = molecules(shape, n)
        n_rows = int(routes.route_lengths(mn, me).sum())
        dn, de = torch.from_numpy(mn).cuda(), torch.from_numpy(me).cuda()
        _, constants = bench.workload_constants("cuda", shape)
        torch.manual_seed(0)
        model = mpnn.GGNN(constants).cuda().eval()
        model.sync_free = True
        modes = {"kernels": lambda: LL.molecule_log_likelihood(model, dn, de, add, conn, batch_rows=BATCH_ROWS,
                                                               n_rows=n_rows),
                 "restatement": lambda: restatement(model, dn, de, add, conn, n_rows)}
        with torch.no_grad():
            outs = {k: timed(f)[0] for k, f in modes.items()}         # warm-up
            runs = {k: [] for k in modes}
            for _ in range(a.rounds):
                for k, f in modes.items():
                    runs[k].append(timed(f)[1] * 1000.0 / n)
        diff = float((outs["kernels"] - outs["restatement"]).abs().max())
        W = int(np.prod(add)) + int(np.prod(conn)) + 1
        entry = dict(molecules=n, rows=n_rows, rows_per_molecule=round(n_rows / n, 2), W=W,
                     apd_bytes_not_written=n_rows * W * (1 if n <= 127 else 4), max_abs_difference=diff)
        for k, ms in runs.items():
            entry[k] = dict(ms_per_1000_molecules=round(statistics.median(ms), 3), min=round(min(ms), 3),
                            max=round(max(ms), 3))
            print(f"{shape:7s} {k:12s} {entry[k]['ms_per_1000_molecules']:9.3f} ms per 1000 molecules "
                  f"[{entry[k]['min']:.3f} - {entry[k]['max']:.3f}]  ({n} molecules, {n_rows} rows, W = {W})")
        print(f"{shape:7s} largest |kernels - restatement| over the molecules: {diff:.3e}")
        result["shapes"][shape] = entry
        for rows in (1000, 16000) if shape == "gdb13" else (1000, 4000):
            result["row_kernels"].append(row_kernels(rows, W))
            print("row kernels:", result["row_kernels"][-1])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
