"""Measures the resonance normal form on the device (graphinvent_amd.analyze.resonance / kekulize /
canonical_compound) against ``analyze.validity`` and ``analyze.canonical`` (the kernels that read the same bytes),
against plain ``analyze.unique``, and against a device copy of the inputs.

One device, one process, the variants alternating inside every repetition, device events around the whole Python call:

  resonance            ``analyze.resonance(nodes, edges, None, rules)``                        one launch, edges written
  resonance_no_edges   the same with ``want_edges=False``                                      one launch
  kekulize             ``analyze.kekulize(nodes, r.edges, None, rules)``                        one launch
  canonical_compound   ``analyze.canonical_compound(nodes, edges, None, rules)``                three launches
  unique               ``analyze.unique(nodes, edges)``                                          the identity per labelled graph
  resonance+unique     ``r = resonance(...); unique(nodes, r.edges)``                           the identity per compound
  validity, canonical  ``analyze.validity`` / ``analyze.canonical`` on the same inputs         same bytes read
  copy                 ``nodes.clone(), edges.clone()``                                          the bytes, moved once

at 1000 x 13 (Fe 3) and 250 x 88 (Fe 4) on the synthetic molecules of tools/bench_valence.py, 1000 x 72 (the 863 DRD2
fixture molecules read with ``aromatic="kekulize"`` and tiled), and 1024 x 128 twice: SATURATED molecules (the synthetic
ones with every bond single: V' is empty, no search runs) and the POLYACENE ladder of tests/test_resonance_cpu.py (159
bonds in G', every one delocalised: the worst case the tests hold).  int8 states.  Before timing, the device results are
checked against the specification (tests/resonance_model.py) on the first ``--check-mols`` molecules.

Expectation, from the code only: ``resonance`` on saturated input is within ``validity``'s time plus the written edges
(the read is the same, the row write is a copy): reported as ``resonance - validity`` beside the time of writing
``r.edges`` once (``torch.zeros_like``).  The search-bound rows are reported as measured; no threshold is set.

    python tools/bench_resonance.py [--reps 50] [--check-mols 16] [--out profiles/analyze/resonance.txt]

prints one table and one JSON line and writes both to ``--out``.  There is no CPU path: without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphinvent_amd import analyze  # noqa: E402
from tests import resonance_model as XM  # noqa: E402
from tests import valence_model as VM  # noqa: E402
from tools.bench_valence import ATOMS, CHARGES, event_ms, molecules  # noqa: E402

DRD2_ARGS = dict(atom_types=["C", "N", "O", "F", "S", "Cl", "Br"], formal_charge=[-1, 0, 1], imp_H=[0, 1, 2, 3])


def inputs():
    """(name, nodes, edges (numpy int8), rules arguments)."""
    synth = lambda Fe: dict(atom_types=ATOMS, formal_charge=CHARGES, bond_orders=(1, 2, 3, 1.5)[:Fe])
    yield ("1000x13", *molecules(1000, 13, 3, seed=1013), synth(3))
    yield ("250x88", *molecules(250, 88, 4, seed=338), synth(4))
    rules = analyze.ValenceRules(**DRD2_ARGS)
    parts = [analyze.read_smi(os.path.join(ROOT, "tests", "golden", f), rules, 72, aromatic="kekulize")
             for f in ("drd2_test.smi", "drd2_valid.smi")]
    dn = torch.cat([p.nodes for p in parts]).cpu().numpy()
    de = torch.cat([p.edges for p in parts]).cpu().numpy()
    pick = np.arange(1000) % len(dn)
    yield "1000x72 DRD2", dn[pick], de[pick], DRD2_ARGS
    sn, se = molecules(1024, 128, 4, seed=1152)
    sat = np.zeros_like(se)
    sat[..., 0] = se.any(axis=3)
    yield "1024x128 saturated", sn, sat, synth(4)
    from tests.test_resonance_cpu import polyacene128
    pn, pe = polyacene128()
    yield "1024x128 polyacene", np.repeat(pn[None], 1024, axis=0), np.repeat(pe[None], 1024, axis=0), DRD2_ARGS


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
    ap.add_argument("--check-mols", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resonance needs a GPU: there is no CPU path")
    results, lines = [], []
    for name, hn, he, rule_args in inputs():
        rules = analyze.ValenceRules(**rule_args)
        model = VM.Rules(rule_args["atom_types"], rule_args["formal_charge"], imp_H=rule_args.get("imp_H"),
                         bond_orders=rule_args.get("bond_orders", (1, 2, 3)))
        G, N, Fe = hn.shape[0], hn.shape[1], he.shape[3]
        nodes, edges = torch.from_numpy(hn).cuda(), torch.from_numpy(he).cuda()
        in_bytes = nodes.numel() + edges.numel()
        H = min(args.check_mols, G)
        want = XM.resonance(hn[:H], he[:H], None, model)
        got = analyze.resonance(nodes[:H].contiguous(), edges[:H].contiguous(), None, rules)
        assert all(np.array_equal(got.host()[k], want[k]) for k in got.host()), "resonance differs from the specification"
        assert np.array_equal(got.edges.cpu().numpy(), want["edges"]), "the normal form differs from the specification"
        r = analyze.resonance(nodes, edges, None, rules)
        delocalised, searched = int(r.n_delocalized.sum()), int((r.n_delocalized > 0).sum())
        calls = dict(
            resonance=lambda: analyze.resonance(nodes, edges, None, rules),
            resonance_no_edges=lambda: analyze.resonance(nodes, edges, None, rules, want_edges=False),
            kekulize=lambda: analyze.kekulize(nodes, r.edges, None, rules),
            canonical_compound=lambda: analyze.canonical_compound(nodes, edges, None, rules),
            unique=lambda: analyze.unique(nodes, edges),
            resonance_unique=lambda: analyze.unique(nodes, analyze.resonance(nodes, edges, None, rules).edges),
            validity=lambda: analyze.validity(nodes, edges, None, rules),
            canonical=lambda: analyze.canonical(nodes, edges),
            copy=lambda: (nodes.clone(), edges.clone()),
            write_edges=lambda: torch.zeros_like(r.edges))
        t = timed(calls, args.reps)
        row = dict(kind="resonance", shape=name, G=G, N=N, Fe=Fe, dtype="int8", input_bytes=in_bytes, reps=args.reps,
                   checked_mols=H, delocalised_bonds=delocalised, molecules_with_delocalised_bonds=searched)
        for k, (med, lo, hi) in t.items():
            row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = med, lo, hi
        m = lambda k: row[k + "_ms_median"]
        row["resonance_minus_validity_ms"] = m("resonance") - m("validity")
        row["resonance_over_validity"] = m("resonance") / m("validity")
        row["resonance_unique_over_unique"] = m("resonance_unique") / m("unique")
        results.append(row)
        lines.append(f"{name:>19}: input {in_bytes / 1e6:6.2f} MB, {delocalised} delocalised bonds in {searched} molecules | "
                     f"resonance {m('resonance'):.4f} ms (without edges {m('resonance_no_edges'):.4f}) | kekulize "
                     f"{m('kekulize'):.4f} | canonical_compound {m('canonical_compound'):.4f} | unique {m('unique'):.4f}, "
                     f"resonance + unique {m('resonance_unique'):.4f} ({row['resonance_unique_over_unique']:.2f} x) | validity "
                     f"{m('validity'):.4f} | canonical {m('canonical'):.4f} | copy {m('copy'):.4f} | writing r.edges once "
                     f"{m('write_edges'):.4f} | resonance - validity {row['resonance_minus_validity_ms']:.4f} ms "
                     f"({row['resonance_over_validity']:.2f} x)")
        print(lines[-1], flush=True)
    line = json.dumps({"bench": "resonance", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/bench_resonance.py: the resonance normal form on the device against validity, canonical, unique "
                    "and a device copy of the inputs\n"
                    f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} repetitions in ms, device events "
                    "around the whole Python call, variants alternating; see the tool's docstring for what each column "
                    "is\n\n")
            f.write("\n".join(lines) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
