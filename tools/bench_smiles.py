"""Measures molecule strings on the device (graphinvent_amd.analyze.smiles) against ``analyze.canonical`` and
``analyze.validity`` (the kernels that read exactly the same bytes), a device copy of the same tensors and the host path.

One device, one process, the variants alternating inside every repetition, device events around the whole Python call:

  smiles       ``analyze.smiles(nodes, edges, None, rules)``                       one launch, input order
  smiles_rank  ``analyze.smiles(nodes, edges, None, rules, rank=r)``               one launch, a given rank (canonical's)
  smiles_canon ``analyze.smiles(nodes, edges, None, rules, canonical=True)``       two launches
  canonical    ``analyze.canonical(nodes, edges)``                                 same bytes read: the yardstick
  validity     ``analyze.validity(nodes, edges, None, rules)``                     same bytes read
  copy         ``edges.clone(); nodes.clone()``                                    the rate a device copy reaches
  host         the path being replaced: ``analyze.decode(...).host()`` plus the Python specification per molecule
               (tests/smiles_model.py), timed on the first ``--host-mols`` molecules and quoted per molecule and, scaled
               linearly, per batch.  RDKit's own ``MolToSmiles`` is NOT MEASURED (there is no RDKit to measure)

at 1000 x 13 (Fe 3), 250 x 88 (Fe 4) and 1024 x 128 (Fe 4), int8 and fp32, on the synthetic molecules of
tools/bench_valence.py.  The fourth bond type is read as a second single bond here, not as order 1.5: an aromatic molecule
gets no string and would cost the reading and the checks only; the table says how many strings were written.  Before timing, the device strings are checked against the Python
specification on the timed subset.  Expectation, from the code only: ``smiles`` with a given rank does one depth-first walk
where ``canonical`` does up to 2 N + 2 refinement rounds, so it should take no longer than ``canonical`` in the same run
(10 % margin for the run-to-run spread); the last column says whether it did.

    python tools/bench_smiles.py [--reps 50] [--host-mols 64] [--out profiles/analyze/smiles.txt]

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
from graphinvent_amd import lib as L  # noqa: E402
from tests import smiles_model as SM  # noqa: E402
from tests import valence_model as VM  # noqa: E402
from tools.bench_valence import ATOMS, CHARGES, SHAPES, event_ms, molecules  # noqa: E402


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
        raise SystemExit("bench_smiles needs a GPU: there is no CPU path")
    results, lines = [], []
    for name, G, N, Fn, Fe in SHAPES:
        hn, he = molecules(G, N, Fe, seed=G + N)
        bond_orders = (1, 2, 3, 1)[:Fe]                     # no order 1.5: every molecule is walked and written
        rules = analyze.ValenceRules(ATOMS, CHARGES, bond_orders=bond_orders)
        model = VM.Rules(ATOMS, CHARGES, bond_orders=bond_orders)
        H = min(args.host_mols, G)
        groups = [len(ATOMS), len(CHARGES)]
        for dtype in (torch.int8, torch.float32):
            nodes, edges = torch.from_numpy(hn).cuda().to(dtype), torch.from_numpy(he).cuda().to(dtype)
            in_bytes = nodes.numel() * nodes.element_size() + edges.numel() * edges.element_size()
            sub_n, sub_e = nodes[:H].contiguous(), edges[:H].contiguous()
            n_dev = (sub_n != 0).any(dim=2).sum(dim=1).to(torch.int32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()                        # the host path: records to the host, then one string each
            analyze.decode(sub_n, sub_e, n_dev, groups).host()
            host = SM.write_batch(hn[:H], he[:H], None, model)
            host_ms = (time.perf_counter() - t0) * 1e3
            got = analyze.smiles(sub_n, sub_e, None, rules)
            strings, length, status, atom_pos = got.host()
            assert strings == host["strings"] and np.array_equal(status, host["status"]), "smiles differs from the host path"
            assert np.array_equal(length, host["length"]) and np.array_equal(atom_pos, host["atom_pos"])
            rank = analyze.canonical(nodes, edges).rank
            whole = analyze.smiles(nodes, edges, None, rules).host()
            written = sum(1 for s in whole[0] if s)
            truncated = int((whole[2] & L.SMI_TRUNCATED != 0).sum())
            t = timed({"smiles": lambda: analyze.smiles(nodes, edges, None, rules),
                       "smiles_rank": lambda: analyze.smiles(nodes, edges, None, rules, rank=rank),
                       "smiles_canon": lambda: analyze.smiles(nodes, edges, None, rules, canonical=True),
                       "canonical": lambda: analyze.canonical(nodes, edges),
                       "validity": lambda: analyze.validity(nodes, edges, None, rules),
                       "copy": lambda: (edges.clone(), nodes.clone())}, args.reps)
            row = dict(kind="smiles", shape=name, G=G, N=N, Fn=Fn, Fe=Fe, dtype=str(dtype).split(".")[-1],
                       input_bytes=in_bytes, max_len=got.max_len, strings_written=written, truncated=truncated,
                       reps=args.reps, host_mols=H, host_ms=host_ms, host_ms_per_molecule=host_ms / H,
                       host_ms_scaled_to_batch=host_ms / H * G)
            for k, (med, lo, hi) in t.items():
                row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
                row[k + "_read_GBps"] = in_bytes / (med * 1e-3) / 1e9
            row["smiles_rank_over_canonical"] = row["smiles_rank_ms_median"] / row["canonical_ms_median"]
            row["smiles_over_validity"] = row["smiles_ms_median"] / row["validity_ms_median"]
            row["within_expectation"] = row["smiles_rank_over_canonical"] <= 1.10
            row["host_over_smiles"] = row["host_ms_scaled_to_batch"] / row["smiles_ms_median"]
            results.append(row)
            lines.append(f"{name:>9} {row['dtype']:>7}: input {in_bytes / 1e6:7.2f} MB, {written} of {G} strings "
                         f"({truncated} truncated at {got.max_len} B) | smiles {row['smiles_ms_median']:.4f} ms "
                         f"({row['smiles_read_GBps']:.1f} GB/s) | with rank {row['smiles_rank_ms_median']:.4f} ms | "
                         f"canonical=True {row['smiles_canon_ms_median']:.4f} ms | canonical "
                         f"{row['canonical_ms_median']:.4f} ms | validity {row['validity_ms_median']:.4f} ms | copy "
                         f"{row['copy_ms_median']:.4f} ms ({row['copy_read_GBps']:.1f} GB/s) | host "
                         f"{row['host_ms_per_molecule']:.2f} ms per molecule, {row['host_ms_scaled_to_batch']:.0f} ms scaled "
                         f"to the batch = {row['host_over_smiles']:.0f} x smiles | smiles with rank / canonical "
                         f"{row['smiles_rank_over_canonical']:.2f} ({'within' if row['within_expectation'] else 'OVER'} "
                         f"1.10), smiles / validity {row['smiles_over_validity']:.2f}")
            print(lines[-1], flush=True)
    line = json.dumps({"bench": "smiles", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_smiles.py: molecule strings on the device against canonical, validity, a device copy and "
                    f"the host path\ndevice: {torch.cuda.get_device_name(0)}; medians of {args.reps} repetitions, device "
                    "events around the whole Python call, variants alternating; see the tool's docstring for what each "
                    "column is.  The host path is decode(...).host() plus the Python specification per molecule; RDKit's "
                    "MolToSmiles is NOT MEASURED (no RDKit)\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
