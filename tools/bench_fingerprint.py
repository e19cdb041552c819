"""Measures molecule scoring on the device (graphinvent_amd.analyze.fingerprint / similarity / activity) against
``analyze.validity`` and ``analyze.canonical`` (the kernels that read exactly the same bytes) and against the host path.

One device, one process, the variants alternating inside every repetition, device events around the whole Python call:

  fingerprint  ``analyze.fingerprint(nodes, edges, None, rules, radius=2, n_bits=2048)``       one launch
  validity     ``analyze.validity(nodes, edges, None, rules)``                                    same bytes read
  canonical    ``analyze.canonical(nodes, edges)``                                                same bytes read
  host         the numpy specification per molecule (tests/fingerprint_model.py), timed on the first ``--host-mols``
               molecules and quoted per molecule and, scaled linearly, per batch.  It stands in for the reference's host
               path; RDKit's own Morgan fingerprint + scikit-learn ``predict_proba`` is NOT MEASURED (there is no RDKit
               to measure)

at 1000 x 13 (Fe 3), 250 x 88 (Fe 4) and 1024 x 128 (Fe 4), int8 and fp32, on the synthetic molecules of
tools/bench_valence.py.  Then, for G = 1000 fingerprints of 2048 bits (those of the 1000 x 13 molecules) against a stored
set of S = 64, 1024 and 16384 random rows: ``similarity`` and ``activity`` (RBF and Tanimoto kernel models with random
coefficients), and the numpy model's ``compare`` on the first ``--host-mols`` queries, scaled.  Before timing, the device
results are checked against the numpy model on the timed subset.  Expectation, from the code only: ``fingerprint`` does at
most 4 refinement rounds where ``canonical`` does up to 2 N + 2, so it should take no longer than ``canonical`` in the same
run (10 % margin for the run-to-run spread); the last column says whether it did.  No threshold is set for the set
comparison.

    python tools/bench_fingerprint.py [--reps 50] [--host-mols 64] [--out profiles/analyze/score.txt]

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
from tests import fingerprint_model as FM  # noqa: E402
from tests import valence_model as VM  # noqa: E402
from tools.bench_valence import ATOMS, CHARGES, SHAPES, event_ms, molecules  # noqa: E402

SET_SIZES = (64, 1024, 16384)
N_BITS, RADIUS = 2048, 2


def timed(calls, reps):
    """Medians (and min / max) in ms of every call, the calls alternating inside each repetition."""
    t = {k: [] for k in calls}
    for _ in range(5):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(event_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-mols", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fingerprint needs a GPU: there is no CPU path")
    results, lines, query = [], [], None
    for name, G, N, Fn, Fe in SHAPES:
        hn, he = molecules(G, N, Fe, seed=G + N)
        bond_orders = (1, 2, 3, 1.5)[:Fe]
        rules = analyze.ValenceRules(ATOMS, CHARGES, bond_orders=bond_orders)
        model = VM.Rules(ATOMS, CHARGES, bond_orders=bond_orders)
        H = min(args.host_mols, G)
        t0 = time.perf_counter()
        host = FM.fingerprint(hn[:H], he[:H], None, model, radius=RADIUS, n_bits=N_BITS)
        host_ms = (time.perf_counter() - t0) * 1e3
        for dtype in (torch.int8, torch.float32):
            nodes, edges = torch.from_numpy(hn).cuda().to(dtype), torch.from_numpy(he).cuda().to(dtype)
            in_bytes = nodes.numel() * nodes.element_size() + edges.numel() * edges.element_size()
            got = analyze.fingerprint(nodes[:H].contiguous(), edges[:H].contiguous(), None, rules, radius=RADIUS,
                                      n_bits=N_BITS, atom_ids=True).host()
            assert all(np.array_equal(got[k], host[k]) for k in got), "fingerprint differs from the host path"
            t = timed({"fingerprint": lambda: analyze.fingerprint(nodes, edges, None, rules, radius=RADIUS, n_bits=N_BITS),
                       "validity": lambda: analyze.validity(nodes, edges, None, rules),
                       "canonical": lambda: analyze.canonical(nodes, edges)}, args.reps)
            if query is None:
                query = analyze.fingerprint(nodes, edges, None, rules, radius=RADIUS, n_bits=N_BITS)
            row = dict(kind="fingerprint", shape=name, G=G, N=N, Fn=Fn, Fe=Fe, dtype=str(dtype).split(".")[-1],
                       input_bytes=in_bytes, reps=args.reps, host_mols=H, host_ms=host_ms,
                       host_ms_per_molecule=host_ms / H, host_ms_scaled_to_batch=host_ms / H * G)
            for k, (med, lo, hi) in t.items():
                row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
                row[k + "_read_GBps"] = in_bytes / (med * 1e-3) / 1e9
            row["fingerprint_over_canonical"] = row["fingerprint_ms_median"] / row["canonical_ms_median"]
            row["fingerprint_over_validity"] = row["fingerprint_ms_median"] / row["validity_ms_median"]
            row["within_expectation"] = row["fingerprint_over_canonical"] <= 1.10
            row["host_over_fingerprint"] = row["host_ms_scaled_to_batch"] / row["fingerprint_ms_median"]
            results.append(row)
            lines.append(f"{name:>9} {row['dtype']:>7}: input {in_bytes / 1e6:7.2f} MB | fingerprint "
                         f"{row['fingerprint_ms_median']:.4f} ms ({row['fingerprint_read_GBps']:.1f} GB/s) | validity "
                         f"{row['validity_ms_median']:.4f} ms | canonical {row['canonical_ms_median']:.4f} ms | host "
                         f"{row['host_ms_per_molecule']:.2f} ms per molecule, {row['host_ms_scaled_to_batch']:.0f} ms scaled "
                         f"to the batch = {row['host_over_fingerprint']:.0f} x fingerprint | fingerprint / canonical "
                         f"{row['fingerprint_over_canonical']:.2f} ({'within' if row['within_expectation'] else 'OVER'} "
                         f"1.10), / validity {row['fingerprint_over_validity']:.2f}")
            print(lines[-1], flush=True)
    # the set comparison: G = 1000 fingerprints of the 1000 x 13 molecules against S random rows
    G = len(query)
    hq = query.host()["bits"]
    rng = np.random.default_rng(7)
    H = min(args.host_mols, G)
    for S in SET_SIZES:
        hs = FM.pack(rng.random((S, N_BITS)) < 0.03)
        coef = (rng.standard_normal(S) / S).astype(np.float32)
        ref = analyze.FingerprintSet(hs)
        models = {"rbf": analyze.KernelModel(ref, coef, 0.1, "rbf", gamma=1.0 / 64, prob_a=-2.0, prob_b=0.1),
                  "tanimoto": analyze.KernelModel(ref, coef, 0.1, "tanimoto", prob_a=-2.0, prob_b=0.1)}
        t0 = time.perf_counter()
        host = FM.compare(hq[:H], hs, weight=coef.astype(np.float64), kind="rbf", gamma=1.0 / 64, intercept=0.1,
                          prob_a=-2.0, prob_b=0.1)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = analyze.activity(query, models["rbf"]).host()
        assert all(np.array_equal(got[k][:H], host[k]) for k in ("nearest", "common", "union", "max_sim"))
        assert np.abs(got["decision"][:H] - host["decision"]).max() <= 1e-4 * host["abs_sum"].max()
        t = timed({"similarity": lambda: analyze.similarity(query, ref),
                   "activity_rbf": lambda: analyze.activity(query, models["rbf"]),
                   "activity_tanimoto": lambda: analyze.activity(query, models["tanimoto"])}, args.reps)
        words = G * S * (N_BITS // 32)
        row = dict(kind="compare", G=G, S=S, n_bits=N_BITS, reps=args.reps, and_popcount_words=words, host_mols=H,
                   host_ms=host_ms, host_ms_scaled_to_batch=host_ms / H * G)
        for k, (med, lo, hi) in t.items():
            row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
            row[k + "_Gwords_per_s"] = words / (med * 1e-3) / 1e9
        row["host_over_activity_rbf"] = row["host_ms_scaled_to_batch"] / row["activity_rbf_ms_median"]
        results.append(row)
        lines.append(f"G {G} x S {S:>5} x {N_BITS} bits: similarity {row['similarity_ms_median']:.4f} ms "
                     f"({row['similarity_Gwords_per_s']:.0f} G AND-popcount words/s) | activity rbf "
                     f"{row['activity_rbf_ms_median']:.4f} ms | activity tanimoto {row['activity_tanimoto_ms_median']:.4f} "
                     f"ms | host (numpy model, rbf) {row['host_ms_scaled_to_batch']:.0f} ms scaled to the batch = "
                     f"{row['host_over_activity_rbf']:.0f} x activity")
        print(lines[-1], flush=True)
    line = json.dumps({"bench": "fingerprint", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_fingerprint.py: molecule scoring on the device (fingerprint, similarity, activity) against "
                    "validity, canonical and the host path\n"
                    f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} repetitions, device events around the "
                    "whole Python call, variants alternating; see the tool's docstring for what each column is.  The host "
                    "path is the numpy specification; RDKit's Morgan fingerprint + scikit-learn predict_proba is NOT "
                    "MEASURED (no RDKit)\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
