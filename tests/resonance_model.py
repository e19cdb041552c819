"""Test helper: the pure-Python specification of the resonance normal form (csrc/gi_resonance.hip, ``gi_mol_resonance``
and ``gi_mol_kekulize``; ``graphinvent_amd.analyze.resonance`` / ``kekulize`` / ``canonical_compound``).  The device
must match ``resonance`` and ``kekulize`` in every integer of every output.

THIS IS NOT AROMATICITY PERCEPTION: no Hueckel count, no chemistry table, no moving charges, no tautomers.  It answers
the one question identity needs: WHICH BONDS CHANGE ORDER BETWEEN THE KEKULE STRUCTURES OF THIS MOLECULE.

The rule, for one well-formed molecule of n atoms (the front end is ``valence_model.judge``'s: a malformed bit,
RES_EMPTY or RES_SELF_LOOP and nothing is delocalised; orders from ``rules.order2``):

  d(i)    the number of order-2 bonds at atom i;  t(i) the number of bonds of order 3 or 1.5 at atom i
  V'      the atoms with d = 1 and t = 0 whose double-bond partner (``mate``) also has d = 1 and t = 0
  G'      vertex set V'; its edges are the bonds of order 1 or 2 between two members of V'.  The double bonds inside V'
          are a perfect matching M of G'
  a bond e = (a, b) of G' is DELOCALISED
          order 2: when G' - e (the edge removed) has a perfect matching
          order 1: when G' - a - b (both atoms removed) has a perfect matching
          equivalently: when e lies on an M-alternating cycle.  No other bond is delocalised
  normal form   ``nodes`` unchanged; ``edges`` [N, N, Fe + 1] int8: a delocalised bond has channel Fe set and no other,
          every other set entry is as stored: 1, or 2 throughout a molecule with MOL_VALUE, so that ``canonical`` on
          the normal form reports what it reports on the stored molecule
  RES_AROMATIC  (informational) a stored bond of order 1.5 is in use; it is left as it is and keeps its atoms out of V'

What follows from the rule (tests/test_resonance_cpu.py checks each):
  phase invariance  V' and G' do not depend on the stored phase and the verdict is a property of G', so all Kekule
          structures of one compound (same atoms, charges, hydrogens; the double bonds another perfect matching of G')
          have the same normal form, byte for byte
  converse          equal normal forms: the two stored structures are perfect matchings of one G'
  only ring bonds   an alternating cycle is a cycle: no acyclic bond is delocalised
  valence-neutral   on an alternating cycle every atom has one single and one double bond: the bond-order sum of every
          atom is the same in the stored molecule and in every Kekule structure ``kekulize`` writes

HOW THE VERDICTS ARE FOUND here and on the device (the verdict is definitional, the order of the searches is free):
with M in hand, removing a double bond (a, b) frees a and b, and removing the atoms of a single bond (u, v) frees
mate(u) and mate(v); in both cases the rest has a perfect matching iff ONE augmenting path joins the two free atoms
(``search``, the breadth-first search with blossom contraction of ``kekule_read_model.match``).  The path and what was
removed close an M-alternating cycle, all of whose bonds are delocalised at once.

``kekulize`` is the inverse: edges [N, N, Fe + 1]; an atom NEEDS a double bond when it carries a channel-Fe bond, the
candidate graph is the channel-Fe bonds, ``kekule_read_model.match`` runs exactly as in the reader (greedy in ascending
index, then one search per free atom, neighbours ascending); matched bonds get the first double type, every other
channel-Fe bond the first single type.  No perfect matching: RES_NO_KEKULE; channel-Fe bonds and no single or no double
type in the rules: RES_BOND_ORDER; either of them, a malformed bit, RES_EMPTY or RES_SELF_LOOP: all-zero edges.  The
choice is a function of the indexed graph, so on canonical molecules it is a canonical Kekule structure
(``canonical_compound``: ``resonance`` -> ``canon_model.canonical`` -> ``kekulize``)."""
import numpy as np

from tests import canon_model as CM
from tests import kekule_read_model as KM
from tests import valence_model as VM

RES_EMPTY, RES_SELF_LOOP, RES_AROMATIC = VM.VAL_EMPTY, VM.VAL_SELF_LOOP, VM.VAL_AROMATIC
RES_BOND_ORDER, RES_NO_KEKULE = 1 << 22, 1 << 26
UNSOUND = VM.MALFORMED | RES_EMPTY | RES_SELF_LOOP
KEKULE_ERROR = UNSOUND | RES_BOND_ORDER | RES_NO_KEKULE


def front_end(nodes, edges, n_given, rules):
    """The labelled front end of ``valence_model.judge`` -> (status bits, n)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N = nodes.shape[0]
    A, C, H = rules.groups
    status, n = CM.status_of(nodes, edges, n_given)
    nz_n, nz_e = nodes != 0, edges != 0
    off = [0, A, A + C, A + C + H]
    for s in range(3 if H else 2):
        if (nz_n[:n, off[s]:off[s + 1]].sum(axis=1) != 1).any():
            status |= VM.MOL_ONEHOT
    if (nz_e.sum(axis=2)[~np.eye(N, dtype=bool)] > 1).any():
        status |= VM.MOL_MULTI_BOND
    if nz_e[np.arange(N), np.arange(N)].any():
        status |= RES_SELF_LOOP
    if n == 0:
        status |= RES_EMPTY
    return status, n


def search(n, cand, mate, root):
    """One breadth-first augmenting-path search with blossom contraction from the free atom ``root``: the search of
    ``kekule_read_model.match``, on a matching that is given.  -> (the free atom reached or -1, parent)."""
    used, parent, base = [False] * n, [-1] * n, list(range(n))
    used[root] = True
    queue, head = [root], 0

    def lca(a, b):
        seen = [False] * n
        while True:
            a = base[a]
            seen[a] = True
            if mate[a] < 0:
                break
            a = parent[mate[a]]
        while True:
            b = base[b]
            if seen[b]:
                return b
            b = parent[mate[b]]

    def mark_path(v, b, child, blossom):
        while base[v] != b:
            blossom[base[v]] = blossom[base[mate[v]]] = True
            parent[v] = child
            child = mate[v]
            v = parent[mate[v]]

    while head < len(queue):
        v = queue[head]
        head += 1
        for to in cand[v]:
            if base[v] == base[to] or mate[v] == to:
                continue
            if to == root or (mate[to] >= 0 and parent[mate[to]] >= 0):
                cur = lca(v, to)
                blossom = [False] * n
                mark_path(v, cur, to, blossom)
                mark_path(to, cur, v, blossom)
                for i in range(n):
                    if blossom[base[i]]:
                        base[i] = cur
                        if not used[i]:
                            used[i] = True
                            queue.append(i)
            elif parent[to] < 0:
                parent[to] = v
                if mate[to] < 0:
                    return to, parent
                used[mate[to]] = True
                queue.append(mate[to])
    return -1, parent


def graph_of(edges, n, rules):
    """G' of a well-formed molecule -> (in_v [n] bool, mate [n] (-1 outside V'), adj [n] sorted neighbour lists in G',
    order {(a, b): 1 or 2} of the G' bonds, both ways, aromatic: a stored 1.5 bond is in use)."""
    nz = np.asarray(edges)[:n, :n] != 0
    o2 = np.asarray(rules.order2)
    dbl = nz[:, :, o2 == 4].any(axis=2)
    sgl = nz[:, :, o2 == 2].any(axis=2)
    oth = nz[:, :, (o2 == 6) | (o2 == 3)].any(axis=2)
    ok = (dbl.sum(axis=1) == 1) & (oth.sum(axis=1) == 0)
    partner = [int(np.argmax(dbl[i])) if ok[i] else -1 for i in range(n)]
    in_v = [bool(ok[i] and ok[partner[i]]) for i in range(n)]
    mate = [partner[i] if in_v[i] else -1 for i in range(n)]
    adj = [[j for j in range(n) if in_v[i] and in_v[j] and (dbl[i, j] or sgl[i, j])] for i in range(n)]
    order = {(i, j): 2 if dbl[i, j] else 1 for i in range(n) for j in adj[i]}
    return in_v, mate, adj, order, bool(nz[:, :, o2 == 3].any())


def delocalized_bonds(n, mate, adj, order, counters=None):
    """The delocalised bonds of G' -> a set of (a, b), both ways.  ``counters``: 'searches' and 'cycles' are counted."""
    count = counters if counters is not None else {}
    count.setdefault("searches", 0)
    count.setdefault("cycles", 0)
    found = set()

    def cycle_through(free_a, free_b, removed, banned, closing):
        m = list(mate)
        m[free_a] = m[free_b] = -1
        for r in removed:
            m[r] = -1
        cand = [[j for j in adj[i] if j not in removed and {i, j} != banned] if i not in removed else []
                for i in range(n)]
        count["searches"] += 1
        v, parent = search(n, cand, m, free_a)
        if v < 0:
            return
        assert v == free_b
        count["cycles"] += 1
        bonds = list(closing)
        while v >= 0:                                                       # the augmenting path, as ``match`` walks it
            pv = parent[v]
            bonds.append((v, pv))
            if m[pv] >= 0:
                bonds.append((pv, m[pv]))
            v = m[pv]
        for a, b in bonds:
            found.update(((a, b), (b, a)))

    for a in range(n):                                                      # the double bonds
        b = mate[a]
        if b > a and (a, b) not in found:
            cycle_through(a, b, (), {a, b}, [(a, b)])
    for u in range(n):                                                      # the single bonds between delocalised atoms
        for v in adj[u]:
            if v > u and order[(u, v)] == 1 and (u, v) not in found and (u, mate[u]) in found and (v, mate[v]) in found:
                cycle_through(mate[u], mate[v], (u, v), None, [(mate[u], u), (u, v), (v, mate[v])])
    return found


def components_of(n, bonds):
    """The number of connected components of the graph of ``bonds`` on its own atoms."""
    root = list(range(n))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    for a, b in bonds:
        ra, rb = find(a), find(b)
        root[max(ra, rb)] = min(ra, rb)
    return len({find(a) for a, _ in bonds})


def resonance_one(nodes, edges, n_given, rules, trace=None):
    """One molecule -> dict(status, n_delocalized, n_atoms, n_systems, delocalized [N, 4] int32, edges [N, N, Fe + 1]
    int8).  ``trace``: a dict that receives n, in_v, mate, adj, order, bonds and counters of a well-formed molecule."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N, Fe = edges.shape[0], edges.shape[2]
    assert len(rules.order2) == Fe
    status, n = front_end(nodes, edges, n_given, rules)
    out_e = np.zeros((N, N, Fe + 1), np.int8)
    out_e[:, :, :Fe] = (edges != 0) * (2 if status & VM.MOL_VALUE else 1)
    rows = np.zeros((N, 4), np.uint32)
    bonds = set()
    if not status & UNSOUND:
        in_v, mate, adj, order, aromatic = graph_of(edges, n, rules)
        if aromatic:
            status |= RES_AROMATIC
        counters = {}
        bonds = delocalized_bonds(n, mate, adj, order, counters)
        if trace is not None:
            trace.update(n=n, in_v=in_v, mate=mate, adj=adj, order=order, bonds=bonds, counters=counters)
        for a, b in bonds:
            out_e[a, b, :Fe] = 0
            out_e[a, b, Fe] = 1
            rows[a, b >> 5] |= np.uint32(1 << (b & 31))
    return dict(status=status, n_delocalized=len(bonds) // 2, n_atoms=len({a for a, _ in bonds}),
                n_systems=components_of(N, bonds), delocalized=rows.view(np.int32), edges=out_e)


def kekulize_one(nodes, edges, n_given, rules, trace=None):
    """One molecule in normal form (edges [N, N, Fe + 1]) -> dict(status, edges [N, N, Fe] int8)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N, Fe = edges.shape[0], edges.shape[2] - 1
    assert len(rules.order2) == Fe
    status, n = front_end(nodes, edges, n_given, rules)
    out_e = np.zeros((N, N, Fe), np.int8)
    if not status & UNSOUND:
        o2 = list(rules.order2)
        if any(o == 3 and (edges[:, :, t] != 0).any() for t, o in enumerate(o2)):
            status |= RES_AROMATIC
        marked = edges[:n, :n, Fe] != 0
        need = [bool(marked[i].any()) for i in range(n)]
        cand = [[int(j) for j in np.flatnonzero(marked[i])] for i in range(n)]
        if any(need) and (2 not in o2 or 4 not in o2):
            status |= RES_BOND_ORDER
        counters = {}
        mate = KM.match(n, need, cand, counters)
        if trace is not None:
            trace.update(n=n, need=need, cand=cand, mate=mate, counters=counters)
        if mate is None:
            status |= RES_NO_KEKULE
        if not status & KEKULE_ERROR:
            out_e[:] = edges[:, :, :Fe] != 0
            for a in range(n):
                for b in cand[a]:
                    out_e[a, b, o2.index(4 if mate[a] == b else 2)] = 1
    return dict(status=status, edges=out_e)


def _batch(one, names, nodes, edges, n_nodes, rules, traces):
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    rows = []
    for g in range(len(nodes)):
        trace = {}
        rows.append(one(nodes[g], edges[g], None if n_nodes is None else n_nodes[g], rules, trace))
        if traces is not None:
            traces.append(trace)
    return {k: np.array([r[k] for r in rows], dt).reshape((len(rows),) + shape) for k, dt, shape in names}


def resonance(nodes, edges, n_nodes, rules, traces=None):
    """Batch model of ``analyze.resonance`` -> dict of status / n_delocalized / n_atoms / n_systems [G] int32,
    delocalized [G, N, 4] int32, edges [G, N, N, Fe + 1] int8."""
    N, Fe = np.asarray(edges).shape[1], np.asarray(edges).shape[3]
    return _batch(resonance_one, [("status", np.int32, ()), ("n_delocalized", np.int32, ()), ("n_atoms", np.int32, ()),
                                  ("n_systems", np.int32, ()), ("delocalized", np.int32, (N, 4)),
                                  ("edges", np.int8, (N, N, Fe + 1))], nodes, edges, n_nodes, rules, traces)


def kekulize(nodes, edges, n_nodes, rules, traces=None):
    """Batch model of ``analyze.kekulize`` -> dict of status [G] int32, edges [G, N, N, Fe] int8."""
    N, Fe = np.asarray(edges).shape[1], np.asarray(edges).shape[3] - 1
    return _batch(kekulize_one, [("status", np.int32, ()), ("edges", np.int8, (N, N, Fe))], nodes, edges, n_nodes,
                  rules, traces)


def canonical_compound(nodes, edges, n_nodes, rules):
    """Batch model of ``analyze.canonical_compound`` -> dict of nodes [G, N, Fn] int8 (canonical), edges [G, N, N, Fe]
    int8 (the canonical Kekule structure), key [G, 2] uint64 (``canonical``'s key of the normal form), status [G]
    int32 (``resonance``'s, with ``canonical``'s bits and RES_NO_KEKULE / RES_BOND_ORDER of ``kekulize`` added)."""
    r = resonance(nodes, edges, n_nodes, rules)
    can = CM.canonical(np.asarray(nodes), r["edges"], n_nodes)
    k = kekulize(can["nodes"], can["edges"], n_nodes, rules)
    status = r["status"] | can["status"] | (k["status"] & (RES_NO_KEKULE | RES_BOND_ORDER))
    return dict(nodes=can["nodes"], edges=k["edges"], key=can["key"], status=status.astype(np.int32))
