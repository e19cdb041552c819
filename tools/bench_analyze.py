"""Measures the molecule read-out (graphinvent_amd.analyze) against the reference's per-molecule Python loops.

One device, one process, the variants alternating inside every repetition:

  props     ``analyze.molecular_properties``           one launch (+ the zero fill of its totals), device events
  decode    ``analyze.decode``                         one launch, device events
  host      ``analyze.decode(...).host()``             launch + one copy + one synchronisation, host clock
  copy      ``edges.clone(); nodes.clone()``           the rate a device copy of the same tensors reaches, device events
  ref       the torch restatement of the reference's loops on the same device tensors (``Analyzer.py:337-478``'s
            histogram loops and ``graph_to_graph``'s ``nonzero`` / ``.item()`` per node and bond, without RDKit), host
            clock around work that ends in a synchronise; ``--ref-reps`` repetitions (it is slow: that is the point)

at 1000 x 13, Fe 3 (fp32 and int8) and 250 x 88, Fe 4 (fp32), on synthetic molecules (random trees with a few ring
closures, one-hot rows).  The launches' rate is the input bytes (nodes + edges + n_nodes) over the median launch time;
``copy`` moves the same bytes once in and once out, and its rate is quoted as bytes READ per second, the same measure.
Before timing, the read-out is checked against the restatement's results (exactly).

    python tools/bench_analyze.py [--reps 200] [--ref-reps 3] [--out FILE.json]

prints one table and one JSON line.  There is no CPU path: without a GPU it fails."""
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

SHAPES = [("1000x13 fp32", 1000, 13, [5, 3], 3, torch.float32), ("1000x13 int8", 1000, 13, [5, 3], 3, torch.int8),
          ("250x88 fp32", 250, 88, [9, 3, 4, 3], 4, torch.float32)]


def molecules(G, N, groups, Fe, seed):
    rng = np.random.default_rng(seed)
    Fn, off = sum(groups), np.cumsum([0] + groups)
    nodes, edges = np.zeros((G, N, Fn), np.int8), np.zeros((G, N, N, Fe), np.int8)
    n_nodes = rng.integers(max(1, N // 2), N + 1, size=G).astype(np.int8)
    for g in range(G):
        n = int(n_nodes[g])
        for s, size in enumerate(groups):
            nodes[g, np.arange(n), off[s] + rng.integers(size, size=n)] = 1
        for i in range(1, n):
            j, t = int(rng.integers(i)), int(rng.integers(Fe))
            edges[g, i, j, t] = edges[g, j, i, t] = 1
        for _ in range(n // 6):                                       # ring closures
            i, j = (int(x) for x in rng.integers(n, size=2))
            if i != j and not edges[g, i, j].any():
                t = int(rng.integers(Fe))
                edges[g, i, j, t] = edges[g, j, i, t] = 1
    return nodes, edges, n_nodes


def reference_loops(nodes, edges, n_nodes_host, groups):
    """The reference's loops on device tensors: every ``int(...)`` and ``.item()`` is a synchronisation."""
    dev = nodes.device
    G, N, Fn = nodes.shape
    Fe = edges.shape[3]
    n_edges_hist = torch.zeros(10, device=dev)
    for g in range(G):                                                # _get_n_edges_distribution
        e = edges[g]
        for node in range(n_nodes_host[g]):
            d = 0
            for bond in range(Fe):
                d += int(torch.sum(e[node, :, bond]))
            n_edges_hist[min(d, 10) - 1] += 1
    n_nodes_hist = torch.zeros(N + 1, device=dev)
    for g in range(G):                                                # _get_n_nodes_distribution
        n_nodes_hist[n_nodes_host[g]] += 1
    nodes_hist = torch.zeros(Fn, device=dev)
    for g in range(G):                                                # _get_node_feature_distribution
        nodes_hist += torch.sum(nodes[g], dim=0)
    edge_hist = torch.zeros(Fe, device=dev)
    for g in range(G):                                                # _get_edge_feature_distribution
        for bond in range(Fe):
            edge_hist[bond] += torch.sum(edges[g][:, :, bond]) / 2
    mask = torch.triu(torch.ones((N, N), device=dev), diagonal=1).view(N, N, 1)
    off = np.cumsum([0] + groups)
    n_atoms = n_bonds = 0
    for g in range(G):                                                # graph_to_graph without RDKit
        for node in range(n_nodes_host[g]):
            idc = torch.nonzero(nodes[g][node])
            _ = [int(idc[k]) - int(off[k]) for k in range(len(groups))]
            n_atoms += 1
        for i, j, t in torch.nonzero(edges[g] * mask):
            _ = (i.item(), j.item(), t.item())
            n_bonds += 1
    torch.cuda.synchronize()
    return n_edges_hist, n_nodes_hist, nodes_hist, edge_hist, n_atoms, n_bonds


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analyze needs a GPU: there is no CPU path")
    results = []
    for name, G, N, groups, Fe, dtype in SHAPES:
        hn, he, hk = molecules(G, N, groups, Fe, seed=G + N)
        nodes, edges = torch.from_numpy(hn).cuda().to(dtype), torch.from_numpy(he).cuda().to(dtype)
        n_nodes, n_host = torch.from_numpy(hk).cuda(), [int(x) for x in hk]
        in_bytes = nodes.numel() * nodes.element_size() + edges.numel() * edges.element_size() + n_nodes.numel()
        # the same results first
        ref = reference_loops(nodes, edges, n_host, groups)
        props = analyze.molecular_properties(nodes, edges, n_nodes, groups)
        atoms, bonds, n_bonds, status = analyze.decode(nodes, edges, n_nodes, groups).host()
        col = torch.cat([props["atom_type_hist"], props["formal_charge_hist"]] +
                        [props[k] for k in ("numh_hist", "chirality_hist") if not isinstance(props[k], list)])
        assert torch.equal(props["n_edges_hist"], ref[0]) and torch.equal(props["n_nodes_hist"], ref[1])
        assert torch.equal(col, ref[2]) and torch.equal(props["edge_feature_hist"], ref[3])
        assert int((atoms[:, :, 0] >= 0).sum()) == ref[4] and int(n_bonds.sum()) == ref[5] and not status.any()
        t = {k: [] for k in ("props", "decode", "host", "copy", "ref")}
        for _ in range(10):                                            # warm-up of every timed variant but ref (done)
            analyze.molecular_properties(nodes, edges, n_nodes, groups)
            analyze.decode(nodes, edges, n_nodes, groups).host()
            edges.clone(), nodes.clone()
        torch.cuda.synchronize()
        for r in range(args.reps):
            t["props"].append(event_ms(lambda: analyze.molecular_properties(nodes, edges, n_nodes, groups)))
            t["decode"].append(event_ms(lambda: analyze.decode(nodes, edges, n_nodes, groups)))
            t0 = time.perf_counter()
            analyze.decode(nodes, edges, n_nodes, groups).host()
            t["host"].append((time.perf_counter() - t0) * 1e3)
            t["copy"].append(event_ms(lambda: (edges.clone(), nodes.clone())))
            if r < args.ref_reps:
                t0 = time.perf_counter()
                reference_loops(nodes, edges, n_host, groups)
                t["ref"].append((time.perf_counter() - t0) * 1e3)
        row = dict(shape=name, G=G, N=N, Fe=Fe, dtype=str(dtype).split(".")[-1], input_bytes=in_bytes, reps=args.reps,
                   ref_reps=len(t["ref"]), atoms=ref[4], bonds=ref[5])
        for k, v in t.items():
            row[k + "_ms_median"] = statistics.median(v)
            row[k + "_ms_min"], row[k + "_ms_max"] = min(v), max(v)
        for k in ("props", "decode", "copy"):
            row[k + "_read_GBps"] = in_bytes / (row[k + "_ms_median"] * 1e-3) / 1e9
        row["ref_over_readout"] = row["ref_ms_median"] / (row["props_ms_median"] + row["host_ms_median"])
        results.append(row)
        print(f"{name:>14}: input {in_bytes / 1e6:7.2f} MB | props {row['props_ms_median']:.4f} ms "
              f"({row['props_read_GBps']:.1f} GB/s) | decode {row['decode_ms_median']:.4f} ms "
              f"({row['decode_read_GBps']:.1f} GB/s) | copy {row['copy_ms_median']:.4f} ms "
              f"({row['copy_read_GBps']:.1f} GB/s) | decode+host {row['host_ms_median']:.3f} ms | reference loops "
              f"{row['ref_ms_median']:.1f} ms = {row['ref_over_readout']:.0f} x (props + decode+host)")
    line = json.dumps({"bench": "analyze", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
