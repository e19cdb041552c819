"""Test helper: the numpy / pure-Python specification of molecule validity on the device (csrc/gi_valence.hip,
``graphinvent_amd.analyze.ValenceRules`` / ``validity`` / ``fraction_valid``).  The device must match it exactly: every
output is an integer or a 0 / 1 float.  It is NOT RDKit and claims no parity with it: a valence test of the labelled
graph, no kekulisation, a table of our own.

The table (``valences_of``): neutral H 1; B 3; C, Si 4; N 3; P 3, 5; O 2; S, Se 2, 4, 6; F, Cl, Br, I 1; group 18: 0.
An atom of group g with charge c in {-1, 0, +1} takes the list of group g - c of its own period (period 2 the first-row
lists, lower periods those of P / S); H+ and H- are 0; anything else has no entry.

The judgement of one molecule with n atoms (``judge``):
  malformed   any of MOL_VALUE, MOL_NODE_PAST_N, MOL_BOND_PAST_N, MOL_ASYMMETRIC (tests/canon_model.status_of),
              MOL_ONEHOT (a row < n without exactly one non-zero entry in the type, charge or implicit-H segment),
              MOL_MULTI_BOND (a pair i != j with several bond types): invalid; atom arrays -1 over all N slots,
              first_bad -1, desc zero, nothing below is evaluated except VAL_EMPTY and VAL_SELF_LOOP
  VAL_EMPTY n == 0;  VAL_SELF_LOOP: some edges[i, i, t] is non-zero
  per atom    o2 = sum_t order2[t] * #{j : edges[i, j, t]}, x = ceil(o2 / 2), v* = the smallest allowed valence >= x;
              none: VAL_OVER, fill 0; else fill h = v* - x; VAL_H_MISMATCH if a stored implicit-H count differs from h
  VAL_AROMATIC a bond type of order 1.5 is in use;  VAL_FRAGMENTS: more than one component
  desc        n_atoms, n_h = sum h + #atoms of type "H", mass_mda = sum mass[type] + sum h * mass_H, n_bonds = #{i < j
              bonded}, n_components, n_rings = n_bonds - n_atoms + n_components
  valid       no malformed bit, not EMPTY, SELF_LOOP, OVER (nor FRAGMENTS under require_connected)"""
import numpy as np

from tests import canon_model as CM

MOL_ONEHOT, MOL_BOND_PAST_N, MOL_VALUE, MOL_MULTI_BOND, MOL_ASYMMETRIC, MOL_NODE_PAST_N = 1, 2, 8, 16, 32, 64
VAL_EMPTY, VAL_SELF_LOOP, VAL_OVER, VAL_FRAGMENTS, VAL_AROMATIC, VAL_H_MISMATCH = 128, 256, 512, 1024, 2048, 4096
MALFORMED = MOL_ONEHOT | MOL_BOND_PAST_N | MOL_VALUE | MOL_MULTI_BOND | MOL_ASYMMETRIC | MOL_NODE_PAST_N
DESC = ("n_atoms", "n_h", "mass_mda", "n_bonds", "n_components", "n_rings")

PERIOD_GROUP = {"B": (2, 13), "C": (2, 14), "N": (2, 15), "O": (2, 16), "F": (2, 17), "Si": (3, 14), "P": (3, 15),
                "S": (3, 16), "Cl": (3, 17), "Se": (4, 16), "Br": (4, 17), "I": (5, 17)}
FIRST_ROW = {13: (3,), 14: (4,), 15: (3,), 16: (2,), 17: (1,), 18: (0,)}
LOWER_ROWS = {13: (3,), 14: (4,), 15: (3, 5), 16: (2, 4, 6), 17: (1,), 18: (0,)}
MASSES = {"H": 1008, "B": 10810, "C": 12011, "N": 14007, "O": 15999, "F": 18998, "Si": 28085, "P": 30974, "S": 32060,
          "Cl": 35450, "Se": 78971, "Br": 79904, "I": 126904}
ORDER2 = {1: 2, 1.5: 3, 2: 4, 3: 6}


def valences_of(symbol, charge):
    """The default table; ``None`` where it has no entry."""
    if charge not in (-1, 0, 1):
        return None
    if symbol == "H":
        return (1,) if charge == 0 else (0,)
    if symbol not in PERIOD_GROUP:
        return None
    period, group = PERIOD_GROUP[symbol]
    return (FIRST_ROW if period == 2 else LOWER_ROWS).get(group - charge)


class Rules:
    """The model's rules: ``allowed[a][c]`` a sorted tuple, ``mass[a]``, ``order2[t]``, ``h_values`` or None."""

    def __init__(self, atom_types, formal_charge, imp_H=None, bond_orders=(1, 2, 3), allowed=None, masses=None):
        allowed = allowed or {}
        masses = dict(MASSES, **(masses or {}))
        self.atom_types, self.formal_charge = list(atom_types), list(formal_charge)
        self.allowed = [[tuple(sorted(allowed.get((a, c)) or valences_of(a, c))) for c in formal_charge]
                        for a in atom_types]
        self.mass = [masses[a] for a in atom_types]
        self.mass_h = masses["H"]
        self.h_type = self.atom_types.index("H") if "H" in self.atom_types else -1
        self.order2 = [ORDER2[b] for b in bond_orders]
        self.h_values = None if imp_H is None else list(imp_H)
        self.groups = (len(self.atom_types), len(self.formal_charge), len(self.h_values or ()))


def components(adj, n):
    """The number of connected components among nodes 0 .. n-1 of a boolean adjacency matrix."""
    seen, comps = np.zeros(n, bool), 0
    for s in range(n):
        if seen[s]:
            continue
        comps += 1
        stack = [s]
        seen[s] = True
        while stack:
            i = stack.pop()
            for j in np.flatnonzero(adj[i, :n] & ~seen):
                seen[j] = True
                stack.append(int(j))
    return comps


def judge(nodes, edges, n_given, rules, require_connected=False):
    """One molecule -> dict(valid, status, first_bad, atom_valence [N], atom_h [N], desc [6])."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N = nodes.shape[0]
    A, C, H = rules.groups
    status, n = CM.status_of(nodes, edges, n_given)
    nz_n, nz_e = nodes != 0, edges != 0
    off = [0, A, A + C, A + C + H]
    for s in range(3 if H else 2):
        if (nz_n[:n, off[s]:off[s + 1]].sum(axis=1) != 1).any():
            status |= MOL_ONEHOT
    pair_types = nz_e.sum(axis=2)
    if (pair_types[~np.eye(N, dtype=bool)] > 1).any():
        status |= MOL_MULTI_BOND
    if nz_e[np.arange(N), np.arange(N)].any():
        status |= VAL_SELF_LOOP
    if n == 0:
        status |= VAL_EMPTY
    out = dict(first_bad=-1, atom_valence=np.full(N, -1, np.int8), atom_h=np.full(N, -1, np.int8),
               desc=np.zeros(6, np.int32))
    if not status & MALFORMED:
        order2 = np.array(rules.order2, np.int64)
        sum_h = n_type_h = mass = 0
        for i in range(n):
            o2 = int((nz_e[i].sum(axis=0) * order2).sum())
            x = (o2 + 1) // 2
            a = int(np.flatnonzero(nz_n[i, :A])[0])
            c = int(np.flatnonzero(nz_n[i, A:A + C])[0])
            fits = [v for v in rules.allowed[a][c] if v >= x]
            out["atom_valence"][i] = min(x, 127)
            if not fits:
                status |= VAL_OVER
                if out["first_bad"] < 0:
                    out["first_bad"] = i
                h = 0
            else:
                h = fits[0] - x
                if H and rules.h_values[int(np.flatnonzero(nz_n[i, A + C:A + C + H])[0])] != h:
                    status |= VAL_H_MISMATCH
            out["atom_h"][i] = h
            sum_h += h
            n_type_h += a == rules.h_type
            mass += rules.mass[a]
        if any(o == 3 and nz_e[:, :, t].any() for t, o in enumerate(rules.order2)):
            status |= VAL_AROMATIC
        bonded = nz_e.any(axis=2)
        n_bonds = int(np.triu(bonded, 1).sum())
        comps = components(bonded, n)
        if comps > 1:
            status |= VAL_FRAGMENTS
        out["desc"][:] = [n, sum_h + n_type_h, mass + sum_h * rules.mass_h, n_bonds, comps, n_bonds - n + comps]
    invalid = MALFORMED | VAL_EMPTY | VAL_SELF_LOOP | VAL_OVER | (VAL_FRAGMENTS if require_connected else 0)
    out.update(status=status, valid=np.float32(0.0 if status & invalid else 1.0))
    return out


def validity(nodes, edges, n_nodes, rules, termination=None, require_connected=False):
    """Batch model of ``analyze.validity`` -> dict of valid [G] fp32, status / first_bad [G] int32, atom_valence /
    atom_h [G, N] int8, desc [G, 6] int32, counts [4] int32."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    G, N = nodes.shape[:2]
    out = dict(valid=np.zeros(G, np.float32), status=np.zeros(G, np.int32), first_bad=np.zeros(G, np.int32),
               atom_valence=np.zeros((G, N), np.int8), atom_h=np.zeros((G, N), np.int8),
               desc=np.zeros((G, 6), np.int32))
    for g in range(G):
        one = judge(nodes[g], edges[g], None if n_nodes is None else n_nodes[g], rules, require_connected)
        for k, v in one.items():
            out[k][g] = v
    term = np.zeros(G, bool) if termination is None else np.asarray(termination) != 0
    ok = out["valid"] != 0
    out["counts"] = np.array([ok.sum(), term.sum(), (ok & term).sum(), G], np.int32)
    return out


def fraction_valid(valid, termination):
    """``Analyzer._get_fraction_valid`` (Analyzer.py:520-544) restated over a validity vector in place of the
    ``SanitizeMol`` calls, in fp32: (fraction_valid, fraction_valid_properly_terminated,
    fraction_properly_terminated)."""
    valid, termination = np.asarray(valid), np.asarray(termination)
    n_graphs = len(valid)
    n_invalid = n_valid_and_properly_terminated = 0
    for idx in range(n_graphs):
        if valid[idx] != 0:
            n_valid_and_properly_terminated += int(termination[idx])
        else:
            n_invalid += 1
    f32 = np.float32
    fraction_valid_ = f32(f32(n_graphs - n_invalid) / f32(n_graphs))
    if 1 in termination:
        fraction_valid_properly_terminated = f32(f32(n_valid_and_properly_terminated) / f32(termination.sum()))
    else:
        fraction_valid_properly_terminated = f32(0.0)
    return fraction_valid_, fraction_valid_properly_terminated, f32(f32(termination.sum()) / f32(len(termination)))


def molecule(N, rules, atoms, bonds, Fn=None, Fe=None):
    """A padded molecule from atoms [(symbol, charge) or (symbol, charge, stored H)] and bonds [(i, j, order)]."""
    A, C, H = rules.groups
    Fn = A + C + H if Fn is None else Fn
    Fe = len(rules.order2) if Fe is None else Fe
    nodes, edges = np.zeros((N, Fn), np.int8), np.zeros((N, N, Fe), np.int8)
    for i, atom in enumerate(atoms):
        nodes[i, rules.atom_types.index(atom[0])] = 1
        nodes[i, A + rules.formal_charge.index(atom[1])] = 1
        if H:
            nodes[i, A + C + rules.h_values.index(atom[2])] = 1
    for i, j, order in bonds:
        t = rules.order2.index(ORDER2[order])
        edges[i, j, t] = edges[j, i, t] = 1
    return nodes, edges
