"""Count the COMPOUNDS of a .smi file, not its Kekule structures, all on the device: no RDKit.

    .smi -> analyze.read_smi(aromatic="kekulize") -> a second copy with the double bonds of every ring system redrawn
         -> analyze.unique on the stored edges            (two Kekule structures of one compound are two classes)
         -> analyze.resonance -> analyze.unique on r.edges (one class per compound)
         -> analyze.canonical_compound -> analyze.smiles   (one string per compound)

    python examples/dedupe_compounds.py [--smi FILE] [--max-n-nodes 72] [--show 5]

Without --smi it reads the committed fixture tests/golden/drd2_test.smi (432 actives of the reference's DRD2 data).

WHAT THIS IS NOT: aromaticity perception.  ``resonance`` finds the bonds that change order between the Kekule structures
of the labelled graph (a bond on a cycle of alternating single and double bonds) and moves them to a channel of their
own; cyclooctatetraene is "delocalised" by that rule, pyrrole is not (it has one Kekule structure, so identity needs
nothing there).  No charges move, no tautomers are merged.  The strings are the library's own spelling of the canonical
Kekule structure, not RDKit's canonical SMILES.

The re-phased copy is made on the host with networkx (a maximum matching with random weights on the delocalised bonds):
it stands in for a generator that draws every ring in whichever phase the draw gives."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphinvent_amd import analyze                               # noqa: E402

ATOM_TYPES, FORMAL_CHARGE, IMP_H = ["C", "N", "O", "F", "S", "Cl", "Br"], [-1, 0, 1], [0, 1, 2, 3]    # the DRD2 sets' parameters


def rephased(edges, delocalized, seed=1):
    """edges [G, N, N, Fe] int8 (numpy) with the double bonds among the delocalised bonds redrawn: another perfect
    matching of them, by networkx with random weights.  Types 0 and 1 are the single and the double bond."""
    import networkx as nx
    rng = random.Random(seed)
    out = edges.copy()
    rows = delocalized.view(np.uint32)
    for g in range(len(edges)):
        graph = nx.Graph()
        for a, w in zip(*np.nonzero(rows[g])):
            for b in range(32 * w, 32 * w + 32):
                if (rows[g, a, w] >> np.uint32(b & 31)) & 1 and a < b:
                    graph.add_edge(int(a), b, weight=rng.random())
        doubles = {frozenset(p) for p in nx.max_weight_matching(graph, maxcardinality=True)}
        for a, b in graph.edges():
            out[g, a, b] = out[g, b, a] = 0
            out[g, a, b, 1 if frozenset((a, b)) in doubles else 0] = out[g, b, a, 1 if frozenset((a, b)) in doubles else 0] = 1
    return out


def run(smi=None, max_n_nodes=72, show=5, verbose=True):
    """-> (molecules, classes of [stored; re-phased] as stored, classes through the normal form, classes of the stored
    half alone, the strings of the stored half, the strings of the re-phased half)."""
    smi = smi or os.path.join(ROOT, "tests", "golden", "drd2_test.smi")
    rules = analyze.ValenceRules(ATOM_TYPES, FORMAL_CHARGE, imp_H=IMP_H)
    mols = analyze.read_smi(smi, rules, max_n_nodes, aromatic="kekulize")
    nodes, edges, n = mols.nodes, mols.edges, mols.n_nodes
    r = analyze.resonance(nodes, edges, n, rules)
    other = torch.from_numpy(rephased(edges.cpu().numpy(), r.host()["delocalized"])).to(edges.device)
    moved = int((other != edges).flatten(1).any(dim=1).sum())
    nodes2, edges2, n2 = torch.cat([nodes, nodes]), torch.cat([edges, other]), torch.cat([n, n])
    valid = analyze.validity(nodes2, edges2, n2, rules).valid
    r2 = analyze.resonance(nodes2, edges2, n2, rules)
    as_stored = int(analyze.unique(nodes2, edges2, n2, mask=valid)[2])
    as_compounds = int(analyze.unique(nodes2, r2.edges, n2, mask=valid)[2])
    half = int(analyze.unique(nodes, r.edges, n, mask=valid[:len(mols)].contiguous())[2])
    cn, ce, _, status = analyze.canonical_compound(nodes2, edges2, n2, rules)
    strings = analyze.smiles(cn, ce, n2, rules).host()[0]
    a, b = strings[:len(mols)], strings[len(mols):]
    if verbose:
        with_bonds = int((r.n_delocalized > 0).sum())
        print(f"{len(mols)} molecules read, {with_bonds} with delocalised bonds, {moved} stored in another phase by the copy")
        print(f"classes of the {2 * len(mols)} molecules [stored; re-phased]: {as_stored} as stored, {as_compounds} through "
              f"the normal form (the stored half alone has {half})")
        print(f"canonical_compound writes the same string for both halves: {a == b}")
        for k in range(min(show, len(mols))):
            print(f"  {a[k]}")
    return len(mols), as_stored, as_compounds, half, a, b


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--smi", default=None)
    ap.add_argument("--max-n-nodes", type=int, default=72)
    ap.add_argument("--show", type=int, default=5)
    args = ap.parse_args()
    run(args.smi, args.max_n_nodes, args.show)
