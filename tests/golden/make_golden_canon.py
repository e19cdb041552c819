"""Golden data for molecule identity (graphinvent_amd.analyze.canonical / unique / SeenSet): our own data, generated
here (``python tests/golden/make_golden_canon.py``).  This script alone imports ``networkx`` (3.4.2 when the file was
written): the expected isomorphism classes come from its VF2 matcher with node-label and bond-type matching, and the
script ASSERTS, on every case it stores, that the classes of the numpy model (tests/canon_model.py) equal VF2's, with
0 disagreements.  The tests then compare the model (CPU) and the device (GPU) with what is stored.

Output ``golden_canon.npz``:

  configs                          gdb13 (N 13), arom5 (N 13, Fe 4), chiral6 (N 40): the fixture molecules of
                                   golden_routes.npz (``c::mol_nodes`` / ``c::mol_edges`` THERE, not copied)
  c::perm [M, 8, N] int8           8 seeded node permutations of every molecule (-1 past n): copy k of molecule m is
                                   ``canon_model.permute(nodes, edges, perm[m, k, :n])``.  Asserted: all 8 have the
                                   model form and key of the original
  c::classes [M] int32             VF2: the lowest index of a molecule isomorphic to m
  c::key [M, 2] uint64             the model's keys (a pin of the model)
  sym::names, sym::nodes [S, 24, 4], sym::edges [S, 24, 24, 3], sym::perm [S, 8, 24], sym::classes, sym::key
                                   symmetric graphs padded into N = 24 (benzene with alternating bond types,
                                   cyclododecane, cubane, prismane, adamantane, decalin, bicyclopentyl,
                                   dodecahedrane, neopentane, tetrahedrane, a 13-path, the Petersen, Desargues and
                                   Moebius-Kantor graphs).  Asserted: ONE model form over 40 seeded node orders each
  miss::names, miss::nodes, miss::edges, miss::perm [S', 8, 24], miss::forms [S']
                                   the known misses (a refinement cell that is not an orbit, no backtracking): the
                                   Frucht graph, the Shrikhande graph, a disconnected C6 + 2 C3 — and cuneane: 3-regular, so
                                   refinement cannot split its 8 atoms, which form THREE orbits (2 + 2 + 4), and the
                                   form depends on the orbit of the atom individualised first.  ``forms`` = distinct
                                   model forms over the original and the 8 stored orders (> 1 for each).  Asserted
                                   only: no form of theirs equals a form of a non-isomorphic graph of sym or miss
  mix::src [B], mix::perm [B, 13], mix::mask [B], mix::rep [B], mix::unique [B]
                                   a mixed batch of gdb13 fixture molecules with planted duplicates (permuted copies,
                                   at distance 1 and B - 1 among them) and a validity mask; rep / unique from VF2
                                   under the semantics of util.py:549-573 (masked-out: unique 1, not remembered)
"""
import os
import sys

import networkx as nx
import numpy as np
from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import canon_model as CM                               # noqa: E402

N_SYM, FN_SYM, FE_SYM = 24, 4, 3
K_STORED, K_TRIED = 8, 40


def to_nx(nodes, edges):
    n = CM.derived_n(nodes)
    g = nx.Graph()
    for i in range(n):
        g.add_node(i, label=nodes[i].tobytes())
    for i in range(n):
        for j in range(i, n):
            t = tuple(np.flatnonzero(edges[i, j]).tolist())
            if t:
                g.add_edge(i, j, bond=t)
    return g


def invariant(g):
    return (g.number_of_nodes(), g.number_of_edges(), tuple(sorted(d["label"] for _, d in g.nodes(data=True))),
            tuple(sorted(d for _, d in g.degree())))


def isomorphic(a, b):
    return invariant(a) == invariant(b) and nx.is_isomorphic(
        a, b, node_match=categorical_node_match("label", None), edge_match=categorical_edge_match("bond", None))


def vf2_classes(graphs):
    rep = []
    for i, g in enumerate(graphs):
        rep.append(next((j for j in range(i) if rep[j] == j and isomorphic(graphs[j], g)), i))
    return np.array(rep, np.int32)


def model_ident(nodes, edges):
    """(key, form bytes) of one molecule under the model."""
    c = CM.canonical(nodes[None], edges[None])
    assert c["status"][0] == 0
    return tuple(c["key"][0].tolist()), c["nodes"][0].tobytes(), c["edges"][0].tobytes()


def model_classes(idents):
    first = {}
    return np.array([first.setdefault(x, i) for i, x in enumerate(idents)], np.int32)


def perms_of(rng, n, N, k):
    out = np.full((k, N), -1, np.int8)
    for q in range(k):
        out[q, :n] = rng.permutation(n)
    return out


def symmetric_graphs():
    def edges_of(g, t=0):
        m = {v: i for i, v in enumerate(g.nodes())}
        return [(m[a], m[b], t) for a, b in g.edges()]
    cuneane = [(a - 1, b - 1, 0) for a, b in ((1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 1), (1, 5),
                                              (2, 4), (3, 7), (6, 8))]
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    adamantane = [(a, 4 + k, 0) for k, (a, b) in enumerate(pairs)] + [(b, 4 + k, 0) for k, (a, b) in enumerate(pairs)]
    decalin = CM.ring(6) + [(0, 6, 0), (6, 7, 0), (7, 8, 0), (8, 9, 0), (9, 5, 0)]
    bicyclopentyl = CM.ring(5) + [(5 + a, 5 + b, t) for a, b, t in CM.ring(5)] + [(0, 5, 0)]
    good = {
        "benzene": (6, [(i, (i + 1) % 6, i % 2) for i in range(6)]),
        "cyclododecane": (12, CM.ring(12)),
        "cubane": (8, edges_of(nx.cubical_graph())),
        "prismane": (6, edges_of(nx.circular_ladder_graph(3))),
        "adamantane": (10, adamantane),
        "decalin": (10, decalin),
        "bicyclopentyl": (10, bicyclopentyl),
        "dodecahedrane": (20, edges_of(nx.dodecahedral_graph())),
        "neopentane": (5, [(0, i, 0) for i in range(1, 5)]),
        "tetrahedrane": (4, CM.complete(4)),
        "path13": (13, CM.path(13)),
        "petersen": (10, edges_of(nx.petersen_graph())),
        "desargues": (20, edges_of(nx.desargues_graph())),
        "moebius_kantor": (16, edges_of(nx.moebius_kantor_graph())),
    }
    shrikhande = [(4 * a + b, 4 * ((a + da) % 4) + (b + db) % 4, 0) for a in range(4) for b in range(4)
                  for da, db in ((1, 0), (0, 1), (1, 1))]
    misses = {
        "cuneane": (8, cuneane),
        "frucht": (12, edges_of(nx.frucht_graph())),
        "shrikhande": (16, shrikhande),
        "c6_2c3": (12, CM.ring(6) + [(6 + a, 6 + b, t) for a, b, t in CM.ring(3)]
                   + [(9 + a, 9 + b, t) for a, b, t in CM.ring(3)]),
    }
    build = lambda d: {k: CM.from_bonds(N_SYM, FN_SYM, FE_SYM, [0] * n, bonds) for k, (n, bonds) in d.items()}
    return build(good), build(misses)


def main():
    R = np.load(os.path.join(HERE, "golden_routes.npz"))
    blob = {"configs": R["configs"]}
    rng = np.random.default_rng(20261019)
    for c in R["configs"]:
        nodes, edges = R[f"{c}::mol_nodes"], R[f"{c}::mol_edges"]
        M, N = nodes.shape[:2]
        idents = [model_ident(nodes[m], edges[m]) for m in range(M)]
        classes = vf2_classes([to_nx(nodes[m], edges[m]) for m in range(M)])
        mine = model_classes(idents)
        assert np.array_equal(mine, classes), (c, int((mine != classes).sum()))
        perm = np.stack([perms_of(rng, CM.derived_n(nodes[m]), N, K_STORED) for m in range(M)])
        for m in range(M):
            n = CM.derived_n(nodes[m])
            for k in range(K_STORED):
                assert model_ident(*CM.permute(nodes[m], edges[m], perm[m, k, :n])) == idents[m], (c, m, k)
        blob.update({f"{c}::perm": perm, f"{c}::classes": classes,
                     f"{c}::key": np.array([i[0] for i in idents], np.uint64)})
        print(f"{c}: {M} molecules, {len(set(classes.tolist()))} classes, model == VF2, 8 orders each: one form")

    good, misses = symmetric_graphs()
    names = list(good)
    nodes, edges = np.stack([good[k][0] for k in names]), np.stack([good[k][1] for k in names])
    idents = [model_ident(nodes[s], edges[s]) for s in range(len(names))]
    graphs = [to_nx(nodes[s], edges[s]) for s in range(len(names))]
    classes = vf2_classes(graphs)
    assert np.array_equal(model_classes(idents), classes) and len(set(classes.tolist())) == len(names)
    perm = []
    for s, name in enumerate(names):
        n = CM.derived_n(nodes[s])
        tried = perms_of(rng, n, N_SYM, K_TRIED)
        forms = {model_ident(*CM.permute(nodes[s], edges[s], p[:n])) for p in tried} | {idents[s]}
        assert len(forms) == 1, (name, len(forms))
        perm.append(tried[:K_STORED])
    blob.update({"sym::names": np.array(names), "sym::nodes": nodes, "sym::edges": edges, "sym::perm": np.stack(perm),
                 "sym::classes": classes, "sym::key": np.array([i[0] for i in idents], np.uint64)})
    print(f"sym: {len(names)} graphs, one form over {K_TRIED} orders each")

    mnames = list(misses)
    mn, me = np.stack([misses[k][0] for k in mnames]), np.stack([misses[k][1] for k in mnames])
    mperm, mforms = [], []
    others = [(idents[s], graphs[s]) for s in range(len(names))]
    mgraphs = [to_nx(mn[s], me[s]) for s in range(len(mnames))]
    all_forms = []
    for s, name in enumerate(mnames):
        n = CM.derived_n(mn[s])
        tried = perms_of(rng, n, N_SYM, K_TRIED)
        every = {model_ident(*CM.permute(mn[s], me[s], p[:n])) for p in tried}
        stored = {model_ident(*CM.permute(mn[s], me[s], p[:n])) for p in tried[:K_STORED]} | {model_ident(mn[s], me[s])}
        print(f"miss {name}: {len(every)} forms over {K_TRIED} orders, {len(stored)} over the stored ones")
        assert len(stored) > 1, name
        mperm.append(tried[:K_STORED])
        mforms.append(len(stored))
        all_forms.append(every | stored)
    for s, forms in enumerate(all_forms):                          # never merged with a non-isomorphic graph
        for ident, g in others:
            assert ident not in forms or isomorphic(g, mgraphs[s])
        for s2, forms2 in enumerate(all_forms):
            assert s2 == s or not (forms & forms2) or isomorphic(mgraphs[s], mgraphs[s2])
    blob.update({"miss::names": np.array(mnames), "miss::nodes": mn, "miss::edges": me, "miss::perm": np.stack(mperm),
                 "miss::forms": np.array(mforms, np.int32)})

    # a mixed batch with planted duplicates and a validity mask
    nodes, edges = R["gdb13::mol_nodes"], R["gdb13::mol_edges"]
    B, N = 64, nodes.shape[1]
    src = rng.choice(24, size=B).astype(np.int32) * 5              # 24 different fixture molecules, repeated
    src[1] = src[0]                                                # distance 1
    src[B - 1] = src[0]                                            # distance B - 1
    perm = np.stack([perms_of(rng, CM.derived_n(nodes[m]), N, 1)[0] for m in src])
    mask = (rng.random(B) < 0.8).astype(np.int8)
    mask[[0, 1, B - 1]] = 1
    mask[5] = 0
    mols = [CM.permute(nodes[m], edges[m], perm[b, :CM.derived_n(nodes[m])]) for b, m in enumerate(src)]
    graphs = [to_nx(a, b) for a, b in mols]
    rep = np.full(B, -1, np.int32)
    for b in range(B):
        if mask[b]:
            rep[b] = next((j for j in range(b) if mask[j] and rep[j] == j and isomorphic(graphs[j], graphs[b])), b)
    uniq = np.where((rep >= 0) & (rep != np.arange(B)), 0.0, 1.0).astype(np.float32)
    can = CM.canonical(np.stack([a for a, _ in mols]), np.stack([b for _, b in mols]))
    u2, r2, counts = CM.unique(can, mask)
    assert np.array_equal(u2, uniq) and np.array_equal(r2, rep), "model != VF2 on the mixed batch"
    assert counts[1] == mask.sum() and counts[2] == (rep == np.arange(B)).sum() and 0 < uniq.sum() < B
    blob.update({"mix::src": src, "mix::perm": perm, "mix::mask": mask, "mix::rep": rep, "mix::unique": uniq})
    print(f"mix: {B} molecules, {int(mask.sum())} masked in, {int(counts[2])} classes")

    out = os.path.join(HERE, "golden_canon.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes; golden_reorder.npz has",
          os.path.getsize(os.path.join(HERE, "golden_reorder.npz")))
    assert os.path.getsize(out) < os.path.getsize(os.path.join(HERE, "golden_reorder.npz"))


if __name__ == "__main__":
    main()
