"""Count functional groups in a .smi file and write the molecules that pass a forbid-list, all on the device: no RDKit.

    .smi -> analyze.read_smi(aromatic="kekulize") -> analyze.substructure (gi_substructure.hip: every molecule against
            every pattern in one launch) -> analyze.substructure_score(forbid=...) -> analyze.smiles -> analyze.write_smi

    python examples/filter_substructures.py [--smi FILE] [--out FILE] [--max-n-nodes 72]

Without --smi it reads the committed fixture tests/golden/drd2_test.smi (432 actives of the reference's DRD2 data).

WHAT THIS IS NOT: the patterns are NOT SMARTS and the matcher is not RDKit's.  A pattern is a molecule-shaped graph —
here written as a SMILES string and read by the library's own reader — whose atoms ask for an element and a charge and
whose bonds ask for a bond type; there are no ring or recursive predicates and NO AROMATICITY IS PERCEIVED.  A ring pattern
read from aromatic SMILES is ONE Kekule phase, so the ring patterns below are built with relax_bonds=True ("any bond
type"), which also lets them match saturated rings of the same elements: cyclohexane counts as "benzene" here.  The
groups are counted as the number of atoms that can play the role of the pattern's FIRST atom (n_anchors)."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphinvent_amd import analyze                               # noqa: E402

ATOM_TYPES, FORMAL_CHARGE, IMP_H = ["C", "N", "O", "F", "S", "Cl", "Br"], [-1, 0, 1], [0, 1, 2, 3]    # the DRD2 sets' parameters
#: counted groups, exact bond types; the first atom of the string is the group's centre
GROUPS = {"amide": "C(=O)N", "carbonyl": "C=O", "nitrile": "C#N", "ether": "COC", "CF3": "C(F)(F)F", "chloride": "ClC",
          "sulfonamide": "S(=O)(=O)N"}
#: ring systems, any bond type on every bond
RINGS = {"six-ring of C": "C1CCCCC1", "piperazine": "N1CCNCC1", "thiophene-like": "C1CCSC1"}
FORBID = ("nitro", "acyl chloride", "long chain")
ALERTS = {"nitro": "[N+](=O)[O-]", "acyl chloride": "C(=O)Cl", "long chain": "CCCCCCCC"}


def pattern_set(rules):
    """The three lists as ONE SubstructureSet; the ring systems ask for any bond type, the rest for theirs."""
    strings = {**GROUPS, **RINGS, **ALERTS}
    return analyze.SubstructureSet.from_smiles(list(strings.values()), rules, max_atoms=8,
                                               relax_bonds=[name in RINGS for name in strings], names=list(strings))


def run(smi=None, out=None, max_n_nodes=72, verbose=True):
    """-> (lines, {group: molecules that contain it}, {group: occurrences}, molecules written, placeholders)."""
    smi = smi or os.path.join(ROOT, "tests", "golden", "drd2_test.smi")
    rules = analyze.ValenceRules(ATOM_TYPES, FORMAL_CHARGE, imp_H=IMP_H)
    patterns = pattern_set(rules)
    mols = analyze.read_smi(smi, rules, max_n_nodes, aromatic="kekulize")
    found = analyze.substructure(mols.nodes, mols.edges, mols.n_nodes, rules, patterns)
    keep = analyze.substructure_score(found, forbid=FORBID)           # fp32 [G] on the device: 1 passes
    valid = analyze.validity(mols.nodes, mols.edges, mols.n_nodes, rules)
    strings = analyze.smiles(mols.nodes, mols.edges, mols.n_nodes, rules)
    with tempfile.TemporaryDirectory() as tmp:
        path = out or os.path.join(tmp, "filtered.smi")
        replaced = analyze.write_smi(path, strings, valid=keep * valid.valid)
    counts = torch.stack([found.match.sum(0), found.n_anchors.sum(0)]).tolist()      # the example's one read-back
    limited = int(found.n_limited.sum())
    contains = dict(zip(patterns.names, counts[0]))
    occurrences = dict(zip(patterns.names, counts[1]))
    if verbose:
        print(f"{len(mols)} molecules, {len(patterns)} patterns, {limited} anchors given up at the step limit")
        for name in patterns.names:
            print(f"  {name:>16}: in {contains[name]:4d} molecules, {occurrences[name]:5d} anchors"
                  f"{'   (forbidden)' if name in FORBID else ''}")
        print(f"{len(mols) - replaced} molecules pass the forbid-list and are written, {replaced} placeholders")
    return len(mols), contains, occurrences, len(mols) - replaced, replaced


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--smi", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-n-nodes", type=int, default=72)
    a = ap.parse_args()
    run(a.smi, a.out, a.max_n_nodes)
