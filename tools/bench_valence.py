"""Measures molecule validity on the device (graphinvent_amd.analyze.validity) against a device copy of the same tensors,
against ``analyze.canonical`` (which reads exactly the same bytes and does more with them) and against the host path.

One device, one process, the variants alternating inside every repetition:

  validity   ``analyze.validity(nodes, edges, None, rules, termination=...)``   one launch, device events around the
             whole Python call
  canonical  ``analyze.canonical(nodes, edges)``                                 the yardstick: same bytes read
  copy       ``edges.clone(); nodes.clone()``                                    the rate a device copy reaches
  host       the path being replaced, on the host: one judgement per molecule (tests/valence_model.py, the numpy
             specification, standing in for RDKit's ``SanitizeMol``); timed on the first ``--host-mols`` molecules and
             quoted per molecule and, scaled linearly, per batch

at 1000 x 13 (Fe 3), 250 x 88 (Fe 4) and 1024 x 128 (Fe 4), int8 and fp32, on synthetic molecules (random trees with a
few ring closures, atom type and charge drawn at random, so part of the atoms are over their valence).  Rates are input
bytes (nodes + edges) over the median time.  Before timing, ``validity`` is checked against the host path's result on the
timed subset.  Expectation: ``validity`` takes no longer than ``canonical`` at each shape in the same run (10 % margin for
the run-to-run spread); the last column says whether it did.

    python tools/bench_valence.py [--reps 50] [--host-mols 64] [--out profiles/analyze/valid.txt]

prints one table and one JSON line and writes both to ``--out``.  There is no CPU path: without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphinvent_amd import analyze  # noqa: E402
from tests import valence_model as VM  # noqa: E402

ATOMS, CHARGES = ["C", "N", "O", "S", "Cl"], [-1, 0, 1]
SHAPES = [("1000x13", 1000, 13, 8, 3), ("250x88", 250, 88, 8, 4), ("1024x128", 1024, 128, 8, 4)]


def molecules(G, N, Fe, seed):
    rng = np.random.default_rng(seed)
    A, C = len(ATOMS), len(CHARGES)
    nodes, edges = np.zeros((G, N, A + C), np.int8), np.zeros((G, N, N, Fe), np.int8)
    for g in range(G):
        n = int(rng.integers(max(1, N // 2), N + 1))
        nodes[g, np.arange(n), rng.choice(A, size=n, p=[0.7, 0.1, 0.1, 0.05, 0.05])] = 1
        nodes[g, np.arange(n), A + rng.choice(C, size=n, p=[0.05, 0.9, 0.05])] = 1
        for i in range(1, n):
            j, t = int(rng.integers(i)), int(rng.choice(Fe, p=[0.8, 0.15, 0.05, 0.0][:Fe] if Fe == 3 else
                                                        [0.75, 0.15, 0.05, 0.05]))
            edges[g, i, j, t] = edges[g, j, i, t] = 1
        for _ in range(n // 6):                                       # ring closures
            i, j = (int(x) for x in rng.integers(n, size=2))
            if i != j and not edges[g, i, j].any():
                edges[g, i, j, 0] = edges[g, j, i, 0] = 1
    return nodes, edges


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-mols", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_valence needs a GPU: there is no CPU path")
    results, lines = [], []
    for name, G, N, Fn, Fe in SHAPES:
        hn, he = molecules(G, N, Fe, seed=G + N)
        bond_orders = (1, 2, 3, 1.5)[:Fe]
        rules = analyze.ValenceRules(ATOMS, CHARGES, bond_orders=bond_orders)
        model = VM.Rules(ATOMS, CHARGES, bond_orders=bond_orders)
        H = min(args.host_mols, G)
        term = (np.arange(G) % 4 != 0).astype(np.int8)
        t0 = time.perf_counter()
        host = VM.validity(hn[:H], he[:H], None, model, termination=term[:H])
        host_ms = (time.perf_counter() - t0) * 1e3
        dterm = torch.from_numpy(term).cuda()
        for dtype in (torch.int8, torch.float32):
            nodes, edges = torch.from_numpy(hn).cuda().to(dtype), torch.from_numpy(he).cuda().to(dtype)
            in_bytes = nodes.numel() * nodes.element_size() + edges.numel() * edges.element_size()
            got = analyze.validity(nodes[:H].contiguous(), edges[:H].contiguous(), None, rules,
                                   termination=dterm[:H].contiguous()).host()
            assert all(np.array_equal(got[k], host[k]) for k in host), "validity differs from the host path"
            n_valid = int(analyze.validity(nodes, edges, None, rules, termination=dterm).host()["counts"][0])
            t = {k: [] for k in ("validity", "canonical", "copy")}
            calls = {"validity": lambda: analyze.validity(nodes, edges, None, rules, termination=dterm),
                     "canonical": lambda: analyze.canonical(nodes, edges),
                     "copy": lambda: (edges.clone(), nodes.clone())}
            for _ in range(5):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for k, fn in calls.items():
                    t[k].append(event_ms(fn))
            row = dict(shape=name, G=G, N=N, Fn=Fn, Fe=Fe, dtype=str(dtype).split(".")[-1], input_bytes=in_bytes,
                       reps=args.reps, valid=n_valid, host_mols=H, host_ms=host_ms, host_ms_per_molecule=host_ms / H,
                       host_ms_scaled_to_batch=host_ms / H * G)
            for k, v in t.items():
                row[k + "_ms_median"] = statistics.median(v)
                row[k + "_ms_min"], row[k + "_ms_max"] = min(v), max(v)
                row[k + "_read_GBps"] = in_bytes / (row[k + "_ms_median"] * 1e-3) / 1e9
            row["validity_over_canonical"] = row["validity_ms_median"] / row["canonical_ms_median"]
            row["within_expectation"] = row["validity_over_canonical"] <= 1.10
            row["host_over_validity"] = row["host_ms_scaled_to_batch"] / row["validity_ms_median"]
            results.append(row)
            lines.append(f"{name:>9} {row['dtype']:>7}: input {in_bytes / 1e6:7.2f} MB, {n_valid} of {G} valid | "
                         f"validity {row['validity_ms_median']:.4f} ms ({row['validity_read_GBps']:.1f} GB/s) | "
                         f"canonical {row['canonical_ms_median']:.4f} ms ({row['canonical_read_GBps']:.1f} GB/s) | copy "
                         f"{row['copy_ms_median']:.4f} ms ({row['copy_read_GBps']:.1f} GB/s) | host "
                         f"{row['host_ms_per_molecule']:.2f} ms per molecule, {row['host_ms_scaled_to_batch']:.0f} ms "
                         f"scaled to the batch = {row['host_over_validity']:.0f} x validity | validity / canonical "
                         f"{row['validity_over_canonical']:.2f} ({'within' if row['within_expectation'] else 'OVER'} 1.10)")
            print(lines[-1], flush=True)
    line = json.dumps({"bench": "valence", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_valence.py: molecule validity on the device against canonical, a device copy and the "
                    f"host path\ndevice: {torch.cuda.get_device_name(0)}; medians of {args.reps} repetitions, device "
                    "events around the whole Python call, variants alternating; see the tool's docstring for what each "
                    "column is\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
