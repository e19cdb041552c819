"""Test helper: the pure-Python specification of substructure search on the device (csrc/gi_substructure.hip,
``graphinvent_amd.analyze.SubstructureSet`` / ``substructure`` / ``substructure_score``).  The device must match it
exactly: every output is an integer.  tests/test_substructure_cpu.py pins it to networkx's monomorphism enumeration.
It is NOT SMARTS and NOT RDKit's matcher: no ring or recursive predicates, no aromaticity perception.

A pattern (``Pattern``) is a connected labelled graph of 1 <= Np <= 32 atoms given as masks: per atom a 0 / 1 row over
the atom types and one over the formal charges (all zero: any; several ones: any of these), per atom pair a 0 / 1 row
over the Fe bond types (all zero: no pattern bond), per atom ``degree`` (the exact number of bonded partners, -1: any)
and ``min_h`` (at least this many hydrogens by the rules' fill, -1: any; an atom over its valence has fill 0, as in
``validity``'s ``atom_h``).

A match is an injective map of the pattern's atoms to molecule atoms < n under which every atom predicate holds and
every pattern bond lands on a molecule bond whose type is in the bond's mask (a monomorphism: the molecule may have
more bonds).  A molecule with a malformed bit, an empty one and one with a self-loop match nothing.

The plan (``plan``): the pattern's atoms in breadth-first order from atom 0, neighbours in ascending index; position
k > 0 has a parent position (the atom it was discovered from) and its other bonds to earlier positions (back bonds,
ascending position).

The search (``search``) of one (molecule, pattern, anchor): the anchor is the image of position 0 (it must satisfy
position 0's predicates; placing it is not a step).  Depth first: at position k the candidates are
``compat[k] & (OR over the bond mask of the adjacency rows of the parent's image) & ~used``, in ascending atom index,
on re-entry after a backtrack only those above the image just abandoned.  TAKING a candidate is one step; then its back
bonds are checked, and a candidate that fails them is abandoned at once.  The search stops at the first full
assignment.  An anchor that is about to take a step when it has already taken ``max_steps`` is given up: no match, and
counted in ``n_limited``."""
import numpy as np

from tests import valence_model as VM

LABEL_BITS = VM.MALFORMED | VM.VAL_EMPTY | VM.VAL_SELF_LOOP
SUB_STEP_LIMIT, SUB_PATTERN_INDEX = 1 << 21, 1 << 22
MAX_PATTERN_ATOMS, MAX_STEPS_LIMIT, DEFAULT_MAX_STEPS = 32, 1 << 20, 4096


class Pattern:
    """type_mask [Np, A], charge_mask [Np, C], bond_mask [Np, Np, Fe] (symmetric), degree / min_h [Np]."""

    def __init__(self, type_mask, charge_mask, bond_mask, degree=None, min_h=None):
        self.type_mask, self.charge_mask = np.asarray(type_mask) != 0, np.asarray(charge_mask) != 0
        self.bond_mask = np.asarray(bond_mask) != 0
        self.Np = len(self.type_mask)
        self.degree = np.full(self.Np, -1) if degree is None else np.asarray(degree)
        self.min_h = np.full(self.Np, -1) if min_h is None else np.asarray(min_h)
        assert 1 <= self.Np <= MAX_PATTERN_ATOMS and (self.bond_mask == self.bond_mask.transpose(1, 0, 2)).all()
        self.order, self.parent, self.back = plan(self.bond_mask.any(axis=2))
        #: types[k][q]: the bond types allowed between the atoms at positions k and q
        self.types = [[[int(t) for t in np.flatnonzero(self.bond_mask[a, b])] for b in self.order] for a in self.order]


def plan(bonded):
    """-> (order [Np]: the pattern atom at every position, parent [Np]: the parent POSITION (0 at position 0),
    back [Np]: the other earlier POSITIONS bonded to it, ascending).  Raises ValueError for a disconnected pattern."""
    Np = len(bonded)
    order, parent_atom, seen = [0], {0: 0}, {0}
    head = 0
    while head < len(order):
        a = order[head]
        head += 1
        for b in range(Np):
            if bonded[a][b] and b != a and b not in seen:
                seen.add(b)
                parent_atom[b] = a
                order.append(b)
    if len(order) != Np:
        raise ValueError("the pattern is not connected")
    pos = {a: k for k, a in enumerate(order)}
    parent = [pos[parent_atom[a]] for a in order]
    back = [sorted(pos[b] for b in range(Np) if bonded[a][b] and b != a and pos[b] < k and pos[b] != parent[k])
            for k, a in enumerate(order)]
    back[0] = []
    return order, parent, back


def from_molecule(nodes, edges, n, rules, relax_bonds=False, any_charge=False):
    """The pattern that asks for molecule (nodes [N, Fn], edges [N, N, Fe]) atom by atom and bond by bond."""
    A, C, _ = rules.groups
    nodes, edges = np.asarray(nodes)[:n], np.asarray(edges)[:n, :n]
    bond = edges != 0
    if relax_bonds:
        bond = np.repeat(bond.any(axis=2, keepdims=True), edges.shape[2], axis=2)
    charge = nodes[:, A:A + C] != 0
    return Pattern(nodes[:, :A] != 0, charge & (not any_charge), bond)


def molecule_state(nodes, edges, n_given, rules):
    """-> (labelled status bits, None) or (0, (n, type [n], charge [n], degree [n], h [n], adj [Fe][n] bit masks))."""
    res = VM.judge(nodes, edges, n_given, rules)
    status = int(res["status"]) & LABEL_BITS
    if status:
        return status, None
    A, C, _ = rules.groups
    n = int(res["desc"][0])
    nz = np.asarray(edges)[:n, :n] != 0
    atype = [int(np.flatnonzero(nodes[i, :A])[0]) for i in range(n)]
    charge = [int(np.flatnonzero(nodes[i, A:A + C])[0]) for i in range(n)]
    degree = nz.any(axis=2).sum(axis=1).tolist()
    adj = [[sum(1 << int(j) for j in np.flatnonzero(nz[i, :, t])) for i in range(n)] for t in range(nz.shape[2])]
    return 0, (n, atype, charge, degree, res["atom_h"][:n].tolist(), adj)


def compat_masks(pattern, state):
    """compat[k]: the molecule atoms that satisfy the predicates of the pattern atom at position k, as a bit mask."""
    n, atype, charge, degree, h, _ = state
    atype, charge, degree, h = (np.asarray(x, np.int64) for x in (atype, charge, degree, h))
    out = []
    for a in pattern.order:
        tm, cm, deg, mh = pattern.type_mask[a], pattern.charge_mask[a], int(pattern.degree[a]), int(pattern.min_h[a])
        ok = np.ones(n, bool)
        if tm.any():
            ok &= tm[atype]
        if cm.any():
            ok &= cm[charge]
        if deg >= 0:
            ok &= degree == deg
        if mh >= 0:
            ok &= h >= mh
        out.append(sum(1 << int(i) for i in np.flatnonzero(ok)))
    return out


def search(pattern, compat, adj, anchor, max_steps):
    """-> (found, img [Np] by POSITION or None, steps, limited)."""
    Np = pattern.Np
    img, used = [anchor] + [-1] * (Np - 1), 1 << anchor
    if Np == 1:
        return True, img, 0, False
    masks = pattern.types
    k, low, steps = 1, -1, 0
    while True:
        par = pattern.parent[k]
        near = 0
        for t in masks[k][par]:
            near |= adj[t][img[par]]
        cand = compat[k] & near & ~used & ~((1 << (low + 1)) - 1)
        if cand == 0:                                        # nothing left at this position: back to the one before
            k -= 1
            if k == 0:
                return False, None, steps, False
            low = img[k]
            used &= ~(1 << low)
            continue
        if steps == max_steps:
            return False, None, steps, True
        steps += 1
        c = (cand & -cand).bit_length() - 1
        if not all(any((adj[t][c] >> img[q]) & 1 for t in masks[k][q]) for q in pattern.back[k]):
            low = c
            continue
        img[k] = c
        used |= 1 << c
        if k == Np - 1:
            return True, img, steps, False
        k, low = k + 1, -1


def match_one(pattern, state, max_steps=DEFAULT_MAX_STEPS, steps_out=None):
    """One (molecule, pattern) -> (match, n_anchors, anchors as a bit mask, first [Np] by pattern atom or None,
    n_limited).  ``steps_out`` (a list) gets (anchor, steps) of every anchor that was tried."""
    n, adj = state[0], state[5]
    compat = compat_masks(pattern, state)
    anchors, first, n_limited = 0, None, 0
    for a in range(n):
        if not (compat[0] >> a) & 1:
            continue
        found, img, steps, limited = search(pattern, compat, adj, a, max_steps)
        if steps_out is not None:
            steps_out.append((a, steps))
        n_limited += limited
        if found:
            anchors |= 1 << a
            if first is None:
                first = [0] * pattern.Np
                for k, atom in enumerate(pattern.order):
                    first[atom] = img[k]
    return int(anchors != 0), bin(anchors).count("1"), anchors, first, n_limited


def substructure(nodes, edges, n_nodes, rules, patterns, pattern_index=None, max_steps=DEFAULT_MAX_STEPS):
    """Batch model of ``analyze.substructure`` -> dict of match / n_anchors / n_limited [G, P] int32, anchors [G, P, 4]
    int32 (bit j of word w: atom 32 w + j), first [G, P, Np_max] int32, status [G] int32; with ``pattern_index`` [G]
    the P axis has length 1."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    G, P = len(nodes), len(patterns)
    Pout, Npm = (P if pattern_index is None else 1), max(p.Np for p in patterns)
    out = dict(match=np.zeros((G, Pout), np.int32), n_anchors=np.zeros((G, Pout), np.int32),
               anchors=np.zeros((G, Pout, 4), np.int32), first=np.full((G, Pout, Npm), -1, np.int32),
               n_limited=np.zeros((G, Pout), np.int32), status=np.zeros(G, np.int32))
    for g in range(G):
        status, state = molecule_state(nodes[g], edges[g], None if n_nodes is None else n_nodes[g], rules)
        todo = list(range(P))
        if pattern_index is not None:
            todo = [int(pattern_index[g])]
            if not 0 <= todo[0] < P:
                status |= SUB_PATTERN_INDEX
                todo = []
        if state is not None:
            for col, p in enumerate(todo):
                m, cnt, anchors, first, lim = match_one(patterns[p], state, max_steps)
                out["match"][g, col], out["n_anchors"][g, col], out["n_limited"][g, col] = m, cnt, lim
                out["anchors"][g, col] = np.array([(anchors >> (32 * w)) & 0xffffffff for w in range(4)],
                                                  np.uint32).view(np.int32)
                if first is not None:
                    out["first"][g, col, :len(first)] = first
                if lim:
                    status |= SUB_STEP_LIMIT
        out["status"][g] = status
    return out


def score(match, require=(), forbid=()):
    """``analyze.substructure_score`` restated: 1.0 where every ``require`` column matches and no ``forbid`` one."""
    ok = np.ones(len(match), bool)
    for p in require:
        ok &= match[:, p] != 0
    for p in forbid:
        ok &= match[:, p] == 0
    return ok.astype(np.float32)
