"""Measures SMILES reading on the device (graphinvent_amd.analyze.read_smiles) against the writer in the same run
(``analyze.smiles`` on the same molecules), a device copy of the reader's own outputs and the host path.

One device, one process, the variants alternating inside every repetition, device events around the whole Python call:

  read       ``analyze.read_smiles(text, rules, N, length=length)``   one launch; the text is the writer's own result,
                                                                      already on the device
  read_list  ``analyze.read_smiles(list of str, rules, N)``           the same plus ``pack_strings`` (one host buffer,
                                                                      one upload) — what ``read_smi`` pays per batch
  rows       ``read`` on G one-atom strings of the same shape         the cost that does not depend on the strings:
                                                                      the launch and the N^2 Fe bytes of every row
  smiles     ``analyze.smiles(nodes, edges, None, rules)``            the writer on the same molecules: the yardstick
  copy       ``nodes.clone(); edges.clone()`` of the reader's result  the rate a device copy of its outputs reaches
  host       the path being replaced: the Python specification per string (tests/smiles_read_model.py), timed on the
             first ``--host-mols`` strings and quoted per string and, scaled linearly, per batch.  RDKit's own
             ``MolFromSmiles`` is NOT MEASURED (there is no RDKit to measure)

at 1000 x 13 (Fe 3), 250 x 88 (Fe 4) and 1024 x 128 (Fe 4), int8, on the strings the writer makes of the synthetic
molecules of tools/bench_valence.py (the fourth bond type read as a second single bond, as in tools/bench_smiles.py).
Before timing, the device result is checked against the Python specification on the timed subset, and the round trip
``smiles(read_smiles(smiles(m)))`` against the first text.  Nobody has measured this before: the tool records, it
promises nothing.  The reader's serial walk is shorter than the writer's, but it writes N^2 Fe bytes per molecule where
the writer writes max_len; the last column says whether ``read`` took more than ``smiles`` plus ``copy``.

    python tools/bench_smiles_read.py [--reps 50] [--host-mols 64] [--out profiles/analyze/smiles_read.txt]

prints one table and one JSON line and writes both to ``--out``.  There is no CPU path: without a GPU it fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphinvent_amd import analyze  # noqa: E402
from graphinvent_amd import lib as L  # noqa: E402
from tests import smiles_read_model as RM  # noqa: E402
from tests import valence_model as VM  # noqa: E402
from tools.bench_smiles import timed  # noqa: E402
from tools.bench_valence import ATOMS, CHARGES, SHAPES, molecules  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-mols", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smiles_read needs a GPU: there is no CPU path")
    results, lines = [], []
    for name, G, N, Fn, Fe in SHAPES:
        hn, he = molecules(G, N, Fe, seed=G + N)
        bond_orders = (1, 2, 3, 1)[:Fe]
        rules = analyze.ValenceRules(ATOMS, CHARGES, bond_orders=bond_orders)
        model = VM.Rules(ATOMS, CHARGES, bond_orders=bond_orders)
        nodes, edges = torch.from_numpy(hn).cuda(), torch.from_numpy(he).cuda()
        written = analyze.smiles(nodes, edges, None, rules)
        strings, w_length, w_status, _ = written.host()
        text, length = written.text, written.length
        H = min(args.host_mols, G)
        t0 = time.perf_counter()                            # the host path: the Python specification per string
        host = RM.read_batch(text[:H].cpu().numpy(), w_length[:H], model, N, Fn, Fe)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = analyze.read_smiles(text[:H].contiguous(), rules, N, length=length[:H].contiguous(), n_bond_types=Fe)
        for k, v in zip(("nodes", "edges", "n_nodes", "status", "atom_pos"), got.host()):
            assert np.array_equal(v, host[k]), f"read_smiles differs from the host path in {k}"
        whole = analyze.read_smiles(written, rules, N, n_bond_types=Fe)
        again = analyze.smiles(whole.nodes, whole.edges, whole.n_nodes, rules)
        has = (written.status & analyze.NO_STRING_BITS) == 0                      # a truncated molecule has no text to read
        assert torch.equal(again.text[has], text[has]) and torch.equal(again.length[has], length[has]), \
            "the round trip changes the text"
        read = int(((whole.status & L.SMR_ERROR) == 0).sum())
        out_bytes = whole.nodes.numel() + whole.edges.numel()
        one_atom, one_length = analyze.pack_strings(["C"] * G, max_len=written.max_len)
        t = timed({"read": lambda: analyze.read_smiles(text, rules, N, length=length, n_bond_types=Fe),
                   "rows": lambda: analyze.read_smiles(one_atom, rules, N, length=one_length, n_bond_types=Fe),
                   "read_list": lambda: analyze.read_smiles(strings, rules, N, n_bond_types=Fe),
                   "smiles": lambda: analyze.smiles(nodes, edges, None, rules),
                   "copy": lambda: (whole.nodes.clone(), whole.edges.clone())}, args.reps)
        row = dict(kind="smiles_read", shape=name, G=G, N=N, Fn=Fn, Fe=Fe, dtype="int8", output_bytes=out_bytes,
                   text_bytes=text.numel(), max_len=written.max_len, mean_length=float(np.mean(w_length)),
                   strings_read=read, reps=args.reps, host_mols=H, host_ms=host_ms, host_ms_per_string=host_ms / H,
                   host_ms_scaled_to_batch=host_ms / H * G)
        for k, (med, lo, hi) in t.items():
            row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
        row["read_write_GBps"] = out_bytes / (row["read_ms_median"] * 1e-3) / 1e9
        row["copy_write_GBps"] = out_bytes / (row["copy_ms_median"] * 1e-3) / 1e9
        row["read_over_smiles"] = row["read_ms_median"] / row["smiles_ms_median"]
        row["read_over_smiles_plus_copy"] = row["read_ms_median"] / (row["smiles_ms_median"] + row["copy_ms_median"])
        row["host_over_read"] = row["host_ms_scaled_to_batch"] / row["read_ms_median"]
        results.append(row)
        lines.append(f"{name:>9}    int8: output {out_bytes / 1e6:7.2f} MB, text {text.numel() / 1e6:.2f} MB (mean "
                     f"{row['mean_length']:.0f} of {written.max_len} B), {read} of {G} strings read | read "
                     f"{row['read_ms_median']:.4f} ms ({row['read_write_GBps']:.1f} GB/s written) | from a list "
                     f"{row['read_list_ms_median']:.4f} ms | one-atom strings {row['rows_ms_median']:.4f} ms | smiles {row['smiles_ms_median']:.4f} ms | copy "
                     f"{row['copy_ms_median']:.4f} ms ({row['copy_write_GBps']:.1f} GB/s) | host "
                     f"{row['host_ms_per_string']:.2f} ms per string, {row['host_ms_scaled_to_batch']:.0f} ms scaled to "
                     f"the batch = {row['host_over_read']:.0f} x read | read / smiles {row['read_over_smiles']:.2f}, read / "
                     f"(smiles + copy) {row['read_over_smiles_plus_copy']:.2f} "
                     f"({'within' if row['read_over_smiles_plus_copy'] <= 1.0 else 'OVER'})")
        print(lines[-1], flush=True)
    line = json.dumps({"bench": "smiles_read", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_smiles_read.py: SMILES reading on the device against the writer in the same run, a device "
                    f"copy of its own outputs and the host path\ndevice: {torch.cuda.get_device_name(0)}; medians of "
                    f"{args.reps} repetitions, device events around the whole Python call, variants alternating; see the "
                    "tool's docstring for what each column is.  The host path is the Python specification per string; "
                    "RDKit's MolFromSmiles is NOT MEASURED (no RDKit)\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
