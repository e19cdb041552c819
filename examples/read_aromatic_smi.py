"""An aromatic .smi file into Kekule molecules and back into a Kekule .smi file, all on the device: no RDKit.

    .smi -> analyze.read_smi(aromatic="kekulize") (gi_smiles_read.hip: the matching inside the reader's one launch)
         -> analyze.validity (gi_valence.hip) -> analyze.smiles (gi_smiles.hip) -> analyze.write_smi

    python examples/read_aromatic_smi.py [--smi FILE] [--out FILE] [--max-n-nodes 72]

Without --smi it reads the committed fixture tests/golden/drd2_test.smi: 432 actives of the reference's DRD2 fine-tuning
data, 430 of them written with aromatic atoms.

WHAT THIS IS NOT: the kekulisation is the library's own rule (a perfect matching of the atoms that need a double bond,
chosen deterministically), NOT RDKit's: no aromaticity perception, no canonical Kekule choice, so two spellings of one
compound can give two different Kekule structures, and what is written is Kekule SMILES, never aromatic SMILES.  A
string without a Kekule structure, or with a stereo mark, comes back as the empty molecule with its status bit."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphinvent_amd import analyze                               # noqa: E402
from graphinvent_amd import lib as L                              # noqa: E402

ATOM_TYPES, FORMAL_CHARGE, IMP_H = ["C", "N", "O", "F", "S", "Cl", "Br"], [-1, 0, 1], [0, 1, 2, 3]    # the DRD2 sets' parameters


def run(smi=None, out=None, max_n_nodes=72, verbose=True):
    """-> (lines, molecules read, of them kekulised, of them valid, placeholders written)."""
    smi = smi or os.path.join(ROOT, "tests", "golden", "drd2_test.smi")
    rules = analyze.ValenceRules(ATOM_TYPES, FORMAL_CHARGE, imp_H=IMP_H)
    mols = analyze.read_smi(smi, rules, max_n_nodes, aromatic="kekulize")
    valid = analyze.validity(mols.nodes, mols.edges, mols.n_nodes, rules)
    strings = analyze.smiles(mols.nodes, mols.edges, mols.n_nodes, rules)
    read = (mols.status & L.SMR_READ_ERROR) == 0                  # still on the device
    counts = torch.stack([read.sum(), ((mols.status & L.SMR_KEKULIZED) != 0).sum(),
                          (read & (valid.valid > 0)).sum()]).tolist()             # the example's one read-back
    with tempfile.TemporaryDirectory() as tmp:
        path = out or os.path.join(tmp, "kekule.smi")
        replaced = analyze.write_smi(path, strings, valid=valid.valid)
        with open(path) as f:
            first = f.read().splitlines()[1:4]
    if verbose:
        print(f"{len(mols)} lines, {counts[0]} read ({counts[1]} kekulised), {counts[2]} valid, {replaced} placeholders")
        for k, s in enumerate(mols.status.tolist()):
            if s & L.SMR_READ_ERROR:
                print(f"  line {k}: {analyze.describe_read_status(s)}")
        print("\n".join("  " + line for line in first))
    return len(mols), counts[0], counts[1], counts[2], replaced


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--smi", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-n-nodes", type=int, default=72)
    a = ap.parse_args()
    run(a.smi, a.out, a.max_n_nodes)
