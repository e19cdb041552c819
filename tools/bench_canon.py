"""Measures molecule identity on the device (graphinvent_amd.analyze.canonical / unique) against the host path it
replaces and against a device copy of the same tensors.

One device, one process, the variants alternating inside every repetition:

  canonical  ``analyze.canonical(..., want_molecules=True)``   one launch, device events
  unique     ``analyze.unique``                                canonical + table insert + finish, device events
  copy       ``edges.clone(); nodes.clone()``                  the rate a device copy of the same tensors reaches
  host       the path being replaced, on the host: per molecule a canonical form (tests/canon_model.py, the numpy
             specification, standing in for RDKit's canonical SMILES) and the reference's ``form in list`` search
             (util.py:549-585); timed on the first ``--host-mols`` molecules and quoted per molecule and, scaled, per
             batch (the list search is quadratic, so the scaled figure flatters the host)

at 1000 x 13 (Fe 3), 250 x 88 (Fe 4) and 1024 x 128 (Fe 4), int8 and fp32, on synthetic molecules (random trees with a
few ring closures, one-hot rows); every second molecule is a node-permuted copy of the one before it, so half of the
batch are duplicates.  Rates are input bytes (nodes + edges) over the median time; ``copy`` is quoted as bytes READ per
second, the same measure.  Before timing, ``unique`` is checked against the host path's result on the timed subset.

    python tools/bench_canon.py [--reps 100] [--host-mols 64] [--out profiles/analyze/unique.txt]

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
from tests import canon_model as CM  # noqa: E402

SHAPES = [("1000x13", 1000, 13, 8, 3), ("250x88", 250, 88, 19, 4), ("1024x128", 1024, 128, 19, 4)]


def molecules(G, N, Fn, Fe, seed):
    rng = np.random.default_rng(seed)
    nodes, edges = np.zeros((G, N, Fn), np.int8), np.zeros((G, N, N, Fe), np.int8)
    for g in range(0, G, 2):
        n = int(rng.integers(max(1, N // 2), N + 1))
        nodes[g, np.arange(n), rng.integers(Fn, size=n)] = 1
        for i in range(1, n):
            j, t = int(rng.integers(i)), int(rng.integers(Fe))
            edges[g, i, j, t] = edges[g, j, i, t] = 1
        for _ in range(n // 6):                                       # ring closures
            i, j = (int(x) for x in rng.integers(n, size=2))
            if i != j and not edges[g, i, j].any():
                t = int(rng.integers(Fe))
                edges[g, i, j, t] = edges[g, j, i, t] = 1
        if g + 1 < G:
            nodes[g + 1], edges[g + 1] = CM.permute(nodes[g], edges[g], rng.permutation(n))
    return nodes, edges


def host_path(nodes, edges):
    """The reference's loop (util.py:549-573) with the model's canonical form in place of the SMILES string."""
    seen, uniq = [], []
    for g in range(len(nodes)):
        n = CM.derived_n(nodes[g])
        a, b = CM.form_of(nodes[g], edges[g], CM.canonical_order(nodes[g], edges[g], n))
        form = (a.tobytes(), b.tobytes())
        uniq.append(0.0 if form in seen else 1.0)
        seen.append(form)
    return np.array(uniq, np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-mols", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_canon needs a GPU: there is no CPU path")
    results, lines = [], []
    for name, G, N, Fn, Fe in SHAPES:
        hn, he = molecules(G, N, Fn, Fe, seed=G + N)
        H = min(args.host_mols, G)
        t0 = time.perf_counter()
        host_uniq = host_path(hn[:H], he[:H])
        host_ms = (time.perf_counter() - t0) * 1e3
        for dtype in (torch.int8, torch.float32):
            nodes, edges = torch.from_numpy(hn).cuda().to(dtype), torch.from_numpy(he).cuda().to(dtype)
            in_bytes = nodes.numel() * nodes.element_size() + edges.numel() * edges.element_size()
            uniq, rep, n_classes = analyze.unique(nodes[:H].contiguous(), edges[:H].contiguous())
            assert np.array_equal(uniq.cpu().numpy(), host_uniq), "unique differs from the host path"
            _, _, n_classes = analyze.unique(nodes, edges)
            t = {k: [] for k in ("canonical", "unique", "copy")}
            for _ in range(5):
                analyze.canonical(nodes, edges, want_molecules=True)
                analyze.unique(nodes, edges)
                edges.clone(), nodes.clone()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                t["canonical"].append(event_ms(lambda: analyze.canonical(nodes, edges, want_molecules=True)))
                t["unique"].append(event_ms(lambda: analyze.unique(nodes, edges)))
                t["copy"].append(event_ms(lambda: (edges.clone(), nodes.clone())))
            row = dict(shape=name, G=G, N=N, Fn=Fn, Fe=Fe, dtype=str(dtype).split(".")[-1], input_bytes=in_bytes,
                       reps=args.reps, classes=int(n_classes), host_mols=H, host_ms=host_ms,
                       host_ms_per_molecule=host_ms / H, host_ms_scaled_to_batch=host_ms / H * G)
            for k, v in t.items():
                row[k + "_ms_median"] = statistics.median(v)
                row[k + "_ms_min"], row[k + "_ms_max"] = min(v), max(v)
                row[k + "_read_GBps"] = in_bytes / (row[k + "_ms_median"] * 1e-3) / 1e9
            row["host_over_unique"] = row["host_ms_scaled_to_batch"] / row["unique_ms_median"]
            results.append(row)
            lines.append(f"{name:>9} {row['dtype']:>7}: input {in_bytes / 1e6:7.2f} MB, {row['classes']} classes | "
                         f"canonical {row['canonical_ms_median']:.4f} ms ({row['canonical_read_GBps']:.1f} GB/s) | "
                         f"unique {row['unique_ms_median']:.4f} ms ({row['unique_read_GBps']:.1f} GB/s) | copy "
                         f"{row['copy_ms_median']:.4f} ms ({row['copy_read_GBps']:.1f} GB/s) | host "
                         f"{row['host_ms_per_molecule']:.2f} ms per molecule, {row['host_ms_scaled_to_batch']:.0f} ms "
                         f"scaled to the batch = {row['host_over_unique']:.0f} x unique")
            print(lines[-1], flush=True)
    line = json.dumps({"bench": "canon", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_canon.py: molecule identity on the device against the host path and a device copy\n"
                    f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} repetitions, variants "
                    "alternating; see the tool's docstring for what each column is\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
