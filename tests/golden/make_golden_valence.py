"""Writes golden_valence.npz: what the SMILES strings of the reference's shipped debug set say about its 30 molecules,
for tests/test_valence_cpu.py / test_valence_gpu.py to hold the validity model (tests/valence_model.py) and the device
against.

    python tests/golden/make_golden_valence.py <reference checkout>/data/pre-training/gdb13_1K-debug

Input: {train,valid,test}.smi of that directory (data files: one "SMILES name" row per molecule under a header row).
The script asserts that every string is bracket-free, kekulised (no lower-case atoms) and free of Cl / Br, so that a
few lines of SMILES reading (`read_smiles` below, ours) are enough: atoms C N O S F, bonds - = #, branches, ring-closure
digits.  Per molecule it stores
  {split}::smiles       the string
  {split}::elements     heavy-atom counts in the order of ELEMENTS (the fixture's atom types)
  {split}::ring_pairs   the number of ring-closure digit pairs
  {split}::n_h          the hydrogen count of the organic subset: per atom the smallest of its normal valences (C 4, N 3,
                        O 2, S 2 / 4 / 6, F 1) that is >= its bond-order sum, minus that sum
Molecule k of a split is the k-th row with APDs[:, -1] > 0 of tests/golden/gdb13_1K-debug_{split}.npz; the script checks
that pairing by element counts and ring counts (bonds - atoms + 1, the molecules being connected) before it writes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ELEMENTS = ["C", "N", "O", "S", "Cl"]
NORMAL = {"C": (4,), "N": (3,), "O": (2,), "S": (2, 4, 6), "F": (1,)}
BOND = {"-": 1, "=": 2, "#": 3}


def read_smiles(s):
    """-> (symbols, bonds [(i, j, order)], ring-closure pairs) of a bracket-free, kekulised SMILES string."""
    assert not any(ch in s for ch in "[]@/\\.%+:") and "Cl" not in s and "Br" not in s, s
    symbols, bonds, stack, open_rings = [], [], [], {}
    prev, order, pairs = None, 1, 0
    for ch in s:
        if ch in NORMAL:
            symbols.append(ch)
            if prev is not None:
                bonds.append((prev, len(symbols) - 1, order))
            prev, order = len(symbols) - 1, 1
        elif ch in BOND:
            order = BOND[ch]
        elif ch == "(":
            stack.append(prev)
        elif ch == ")":
            prev = stack.pop()
        elif ch.isdigit():
            if ch in open_rings:
                other, o = open_rings.pop(ch)
                bonds.append((other, prev, max(o, order)))
                pairs += 1
            else:
                open_rings[ch] = (prev, order)
            order = 1
        else:
            raise AssertionError(f"unexpected character {ch!r} in {s!r}")
    assert not stack and not open_rings, s
    return symbols, bonds, pairs


def hydrogens(symbols, bonds):
    total = [0] * len(symbols)
    for i, j, o in bonds:
        total[i] += o
        total[j] += o
    return sum(min(v for v in NORMAL[s] if v >= t) - t for s, t in zip(symbols, total))


def main():
    src = sys.argv[1]
    blob = {"elements_order": np.array(ELEMENTS), "splits": np.array(["train", "valid", "test"])}
    for split in ("train", "valid", "test"):
        rows = [ln.split()[0] for ln in open(os.path.join(src, f"{split}.smi")).read().splitlines()[1:] if ln.strip()]
        d = np.load(os.path.join(HERE, f"gdb13_1K-debug_{split}.npz"))
        whole = np.flatnonzero(d["APDs"][:, -1] > 0)
        assert len(rows) == len(whole) == 10, (split, len(rows), len(whole))
        elements, ring_pairs, n_h = [], [], []
        for k, s in enumerate(rows):
            symbols, bonds, pairs = read_smiles(s)
            elements.append([symbols.count(e) for e in ELEMENTS])
            ring_pairs.append(pairs)
            n_h.append(hydrogens(symbols, bonds))
            nodes, edges = d["nodes"][whole[k]], d["edges"][whole[k]]
            assert nodes[:, :5].sum(axis=0).tolist() == elements[-1], (split, k, s)
            n_bonds = int(edges.any(axis=2).sum()) // 2
            assert n_bonds == len(bonds) and n_bonds - len(symbols) + 1 == pairs, (split, k, s)
            assert sorted(o for _, _, o in bonds) == sorted([1] * (int(edges[:, :, 0].sum()) // 2) +
                                                             [2] * (int(edges[:, :, 1].sum()) // 2) +
                                                             [3] * (int(edges[:, :, 2].sum()) // 2)), (split, k, s)
        blob[f"{split}::smiles"] = np.array(rows)
        blob[f"{split}::elements"] = np.array(elements, np.int32)
        blob[f"{split}::ring_pairs"] = np.array(ring_pairs, np.int32)
        blob[f"{split}::n_h"] = np.array(n_h, np.int32)
        print(split, rows[0], elements[0], ring_pairs[0], n_h[0])
    out = os.path.join(HERE, "golden_valence.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
