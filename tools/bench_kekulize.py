"""Measures what kekulising inside the reader costs (graphinvent_amd.analyze.read_smiles(..., aromatic="kekulize")).

One device, one process, the variants alternating inside every repetition, device events around the whole Python call,
the text already on the device:

  kekulize   ``read_smiles(aromatic text, rules, N, length=length, aromatic="kekulize")``   (a)
  kekule     ``read_smiles(Kekule text, rules, N, length=length, aromatic="error")`` on the strings the writer makes of
             the SAME molecules (``analyze.smiles`` of (a)'s result): the same graphs, no matching             (b)
  parent     (b) through another build of the library (``--parent-lib``, the parent commit's
             libgraphinvent_amd.so): its ``gi_smiles_read`` called with the same pointers                       (c)
  host       the path (a) replaces: the Python specification per string (tests/kekule_read_model.py), timed on the
             first ``--host-mols`` strings and scaled linearly to the batch.  RDKit's ``MolFromSmiles`` + ``Kekulize``
             is NOT MEASURED (there is no RDKit to measure)

on three corpora: the 863 DRD2 strings of tests/golden tiled to G = 1000 at N = 72; the 512 generated ring systems of
tests/test_kekulize_cpu.py at N = 40 (203 of them kekulise; the other 309 end in GI_SMR_KEKULE after a failed search,
and have no Kekule string for (b), which is then timed on the 203 tiled to 512); and 1000 rings of 128 ``c`` at N = 128,
the serial stage's bad case for the greedy pass (64 pairs, no search).  (a) / (b) is what kekulisation costs; (b) / (c)
says whether the untemplated path slowed (the sibling rows allow the 10 % run-to-run spread).  Before timing, (a) is
checked against the specification on the host subset and (b) against (a)'s molecules permuted by ``argsort(atom_pos)``.
The model's counters (greedy pairs, searches, augmentations, blossom contractions per string) say where the serial
stage's time goes.  Nobody has measured this before: the tool records, it promises nothing.

    python tools/bench_kekulize.py [--reps 50] [--host-mols 64] [--parent-lib PATH] [--out profiles/analyze/kekulize.txt]

prints one table and one JSON line and writes both to ``--out``.  There is no CPU path: without a GPU it fails."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphinvent_amd import analyze  # noqa: E402
from graphinvent_amd import lib as L  # noqa: E402
from tests import kekule_read_model as KM  # noqa: E402
from tests import valence_model as VM  # noqa: E402
from tests.test_kekulize_cpu import DRD2_ARGS, drd2_strings, generated_strings  # noqa: E402
from tools.bench_smiles import timed  # noqa: E402


def parent_call(path, rules, text, length, N, Fn, Fe):
    """-> a callable that runs (b) through the library at ``path``: its own gi_smiles_read, the same pointers."""
    lib = ctypes.CDLL(path)
    fn = lib.gi_smiles_read
    fn.restype, fn.argtypes = L.SIGNATURES["gi_smiles_read"]
    A, C, H = rules.groups
    symbols, charges = analyze._smiles_tables("bench_kekulize", rules)
    order2 = rules.order2(Fe)
    G, max_len = text.shape
    res = analyze.ReadMolecules.empty(text.device, G, N, Fn, Fe)
    out = res._ptrs()
    keep = (symbols, charges, order2, res)

    def call():
        rc = fn(G, N, Fn, Fe, text.data_ptr(), length.data_ptr(), max_len, A, C, H, rules.allowed_mask.data_ptr(),
                order2.data_ptr(), rules.h_values.data_ptr(), charges.data_ptr(), symbols.data_ptr(), 0, 0, out["nodes"],
                out["edges"], out["n_nodes"], out["status"], out["atom_pos"], torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return keep
    return call, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-mols", type=int, default=64)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kekulize needs a GPU: there is no CPU path")
    golden = os.path.join(ROOT, "tests", "golden")
    rules, model = analyze.ValenceRules(**DRD2_ARGS), VM.Rules(**DRD2_ARGS)
    Fn, Fe = sum(model.groups), 3
    drd2 = drd2_strings(golden)[0]
    corpora = [("drd2", (drd2 * 2)[:1000], 72), ("generated", generated_strings(), 40),
               ("ring128", ["c1" + "c" * 126 + "c1"] * 1000, 128)]
    results, lines = [], []
    for name, strings, N in corpora:
        G = len(strings)
        text, length = analyze.pack_strings(strings)
        H = min(args.host_mols, G)
        traces = []
        t0 = time.perf_counter()                            # the host path: the Python specification per string
        host = KM.read_batch(strings[:H], None, model, N, aromatic=True, traces=traces)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = analyze.read_smiles(strings[:H], rules, N, aromatic="kekulize")
        for k, v in zip(("nodes", "edges", "n_nodes", "status", "atom_pos"), got.host()):
            assert np.array_equal(v, host[k]), f"read_smiles(kekulize) differs from the specification in {k}"
        counters = {}
        for tr in traces:
            for k, v in (tr.get("counters") or {}).items():
                counters[k] = counters.get(k, 0) + v
        whole = analyze.read_smiles(text, rules, N, length=length, aromatic="kekulize")
        ok = (whole.status & L.SMR_READ_ERROR) == 0
        idx = torch.nonzero(ok).flatten()
        idx = idx[torch.arange(G, device=idx.device) % len(idx)]             # the strings that read, tiled to G
        written = analyze.smiles(whole.nodes[idx].contiguous(), whole.edges[idx].contiguous(),
                                 whole.n_nodes[idx].contiguous(), rules)
        k_text, k_length = written.text, written.length
        back = analyze.read_smiles(k_text, rules, N, length=k_length, aromatic="error")
        assert not bool((back.status & L.SMR_ERROR).any()) and torch.equal(back.n_nodes, whole.n_nodes[idx]), \
            "the Kekule strings do not read back"
        assert int(back.edges.sum()) == int(whole.edges[idx].sum()), "the Kekule strings are other graphs"
        calls = {"kekulize": lambda: analyze.read_smiles(text, rules, N, length=length, aromatic="kekulize"),
                 "kekule": lambda: analyze.read_smiles(k_text, rules, N, length=k_length, aromatic="error")}
        if args.parent_lib:
            # the same entry point of this build with the same bare call, so that (b) / (c) compares launches alone
            calls["kekule_bare"], _ = parent_call(L.LIB_PATH, rules, k_text, k_length, N, Fn, Fe)
            calls["parent"], p_res = parent_call(args.parent_lib, rules, k_text, k_length, N, Fn, Fe)
            calls["parent"]()
            assert torch.equal(p_res.edges, back.edges) and torch.equal(p_res.nodes, back.nodes), "the parent reads otherwise"
        t = timed(calls, args.reps)
        row = dict(kind="kekulize", corpus=name, G=G, N=N, Fn=Fn, Fe=Fe, strings_read=int(ok.sum()), reps=args.reps,
                   mean_length=float(length.float().mean()), kekule_mean_length=float(k_length.float().mean()),
                   host_mols=H, host_ms=host_ms, host_ms_per_string=host_ms / H, host_ms_scaled_to_batch=host_ms / H * G,
                   counters_on_host_mols=counters)
        for k, (med, lo, hi) in t.items():
            row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
        row["kekulize_over_kekule"] = row["kekulize_ms_median"] / row["kekule_ms_median"]
        row["host_over_kekulize"] = row["host_ms_scaled_to_batch"] / row["kekulize_ms_median"]
        tail = ""
        if args.parent_lib:
            row["kekule_bare_over_parent"] = row["kekule_bare_ms_median"] / row["parent_ms_median"]
            tail = (f" | bare gi_smiles_read {row['kekule_bare_ms_median']:.4f} ms, the parent's {row['parent_ms_median']:.4f} ms: "
                    f"(b) / (c) {row['kekule_bare_over_parent']:.2f} "
                    f"({'within' if row['kekule_bare_over_parent'] <= 1.10 else 'OVER'} the 10 % spread)")
        results.append(row)
        lines.append(f"{name:>9} {G}x{N}: {row['strings_read']} of {G} strings read, mean {row['mean_length']:.0f} B | (a) kekulize "
                     f"{row['kekulize_ms_median']:.4f} ms | (b) Kekule strings of the same molecules {row['kekule_ms_median']:.4f} ms"
                     f" | (a) / (b) {row['kekulize_over_kekule']:.2f} | host {row['host_ms_per_string']:.2f} ms per string, "
                     f"{row['host_ms_scaled_to_batch']:.0f} ms scaled to the batch = {row['host_over_kekulize']:.0f} x (a) | "
                     f"model counters on the first {H} strings {counters}{tail}")
        print(lines[-1], flush=True)
    line = json.dumps({"bench": "kekulize", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_kekulize.py: what kekulising inside the SMILES reader costs, against the Kekule strings of the "
                    f"same molecules, the parent build and the host path\ndevice: {torch.cuda.get_device_name(0)}; medians of "
                    f"{args.reps} repetitions, device events around the whole Python call, variants alternating; see the "
                    "tool's docstring for what each column is.  The host path is the Python specification per string; "
                    "RDKit's MolFromSmiles + Kekulize is NOT MEASURED (no RDKit)\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
