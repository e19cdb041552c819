"""CPU: the specification of substructure search (tests/substructure_model.py; the device side is
``analyze.substructure`` / ``gi_mol_substructure``), the host side of ``analyze.SubstructureSet``, the binding and the
Python boundary.  No device compute is issued.

THE MATCHER IS THE LIBRARY'S OWN, NOT SMARTS AND NOT RDKit.  The model is pinned (1) to hand cases with written-out
answers, (2) to networkx's ``GraphMatcher.subgraph_monomorphisms_iter`` — an independent enumeration of every
monomorphism — on the DRD2 fixture molecules and every stored set, (3) to its own defining properties (``first`` is a
match from the lowest anchor, anchors move with the atoms under a renumbering), and (4) at the step limit to recorded
step counts."""
import os
import re

import networkx as nx
import numpy as np
import pytest
import torch
from networkx.algorithms import isomorphism

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import kekule_read_model as KM
from tests import substructure_model as SM
from tests import valence_model as VM
from tests.test_kekulize_cpu import DRD2_ARGS, drd2_model, drd2_rules
from tests.test_valence_cpu import RULE_ARGS, model_rules, stored_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}

#: the 18 patterns searched for in the DRD2 molecules: name -> SMILES (read by the model's reader, aromatic ones into
#: ONE Kekule phase); pattern atom 0 is the first atom of the string
PATTERNS18 = {
    "benzene": "c1ccccc1", "amide": "C(=O)N", "piperazine": "N1CCNCC1", "decane": "CCCCCCCCCC",
    "naphthalene": "c1ccc2ccccc2c1", "phenylpiperazine": "c1ccccc1N1CCNCC1", "CF3": "C(F)(F)F", "carbonyl": "C=O",
    "nitrile": "C#N", "nitro": "[N+](=O)[O-]", "carboxyl": "C(=O)O", "sulfonamide": "S(=O)(=O)N", "ether": "COC",
    "thiophene": "c1ccsc1", "pyridine": "c1ccncc1", "chloride": "CCl", "nitrogen": "N", "indole": "c1ccc2[nH]ccc2c1",
}
STORED_SETS = ("gdb13", "arom5", "chiral6", "atoms_charges", "imp_h_chirality")


def pattern_molecules():
    """The 18 strings as the model's reader reads them (nodes, edges, n_nodes), under the DRD2 rules."""
    if "pm" not in _CACHE:
        out = KM.read_batch(list(PATTERNS18.values()), None, drd2_rules(), 32, aromatic=True)
        assert not (out["status"] & KM.RD_ERROR).any()
        _CACHE["pm"] = out["nodes"], out["edges"], out["n_nodes"]
    return _CACHE["pm"]


def drd2_patterns(relax):
    if ("pat", relax) not in _CACHE:
        nodes, edges, n = pattern_molecules()
        _CACHE[("pat", relax)] = [SM.from_molecule(nodes[i], edges[i], n[i], drd2_rules(), relax_bonds=relax)
                                  for i in range(len(n))]
    return _CACHE[("pat", relax)]


def drd2_molecules(golden_dir):
    """The 863 DRD2 molecules as the model's reader reads them: (nodes [863, 72, 14], edges, n_nodes)."""
    out, _ = drd2_model(golden_dir)
    return out["nodes"], out["edges"], out["n_nodes"]


def drd2_states(golden_dir):
    if "states" not in _CACHE:
        nodes, edges, _ = drd2_molecules(golden_dir)
        _CACHE["states"] = [SM.molecule_state(nodes[g], edges[g], None, drd2_rules())[1] for g in range(len(nodes))]
    return _CACHE["states"]


def atoms_of(rules, symbols):
    """[(symbol, charge 0, [first stored H])] for VM.molecule under any of the stored sets' rules."""
    tail = (rules.h_values[0],) if rules.h_values is not None else ()
    return [(s, 0) + tail for s in symbols]


def set_patterns(c):
    """name -> SM.Pattern for the stored set c, from molecules and from masks; C, N and O are in all the rules."""
    if ("setpat", c) in _CACHE:
        return _CACHE[("setpat", c)]
    r = model_rules(c)
    A, C, _ = r.groups
    Fe = len(r.order2)
    mol = lambda symbols, bonds, **kw: SM.from_molecule(*VM.molecule(8, r, atoms_of(r, symbols), bonds), len(symbols), r,
                                                        **kw)
    ring6 = [(i, (i + 1) % 6, 1) for i in range(6)]
    pats = {
        "CC": mol("CC", [(0, 1, 1)]), "C=O": mol("CO", [(0, 1, 2)]), "CN_relaxed": mol("CN", [(0, 1, 1)], relax_bonds=True),
        "CCO_any_charge": mol("CCO", [(0, 1, 1), (1, 2, 1)], any_charge=True),
        "ring3": mol("CCC", [(0, 1, 1), (1, 2, 1), (0, 2, 1)], relax_bonds=True),
        "branch": mol("CCCC", [(0, 1, 1), (0, 2, 1), (0, 3, 1)]),
        "ring6_relaxed": mol("CCCCCC", ring6, relax_bonds=True),
    }
    any2 = np.zeros((2, 2, Fe), bool)
    any2[0, 1] = any2[1, 0] = True
    pats["any_any"] = SM.Pattern(np.zeros((2, A)), np.zeros((2, C)), any2)
    no = np.zeros((1, A))
    no[0, [r.atom_types.index("N"), r.atom_types.index("O")]] = 1
    pats["N_or_O"] = SM.Pattern(no, np.zeros((1, C)), np.zeros((1, 1, Fe)))
    pats["N_or_O_with_H"] = SM.Pattern(no, np.zeros((1, C)), np.zeros((1, 1, Fe)), min_h=[1])
    ring_any = np.zeros((5, 5, Fe), bool)
    for i in range(5):
        ring_any[i, (i + 1) % 5] = ring_any[(i + 1) % 5, i] = True
    pats["ring5_any_atoms_degree2_at_0"] = SM.Pattern(np.zeros((5, A)), np.zeros((5, C)), ring_any,
                                                     degree=[2, -1, -1, -1, -1])
    _CACHE[("setpat", c)] = pats
    return pats


def stack_patterns(patterns):
    """A list of SM.Pattern as the padded arrays ``analyze.SubstructureSet`` takes."""
    P, Npm = len(patterns), max(p.Np for p in patterns)
    A, C, Fe = patterns[0].type_mask.shape[1], patterns[0].charge_mask.shape[1], patterns[0].bond_mask.shape[2]
    tm, cm, bm = np.zeros((P, Npm, A), np.int8), np.zeros((P, Npm, C), np.int8), np.zeros((P, Npm, Npm, Fe), np.int8)
    deg, mh = np.full((P, Npm), -1), np.full((P, Npm), -1)
    for i, p in enumerate(patterns):
        tm[i, :p.Np], cm[i, :p.Np], bm[i, :p.Np, :p.Np] = p.type_mask, p.charge_mask, p.bond_mask
        deg[i, :p.Np], mh[i, :p.Np] = p.degree, p.min_h
    return dict(type_mask=tm, charge_mask=cm, bond_mask=bm, degree=deg, min_h=mh)


def nx_anchors(pattern, state):
    """networkx's answer: (the molecule atoms that are the image of pattern atom 0 in some monomorphism, as a bit mask)."""
    n, atype, charge, degree, h, adj = state
    M, Q = nx.Graph(), nx.Graph()
    for i in range(n):
        M.add_node(i, a=atype[i], c=charge[i], d=degree[i], h=h[i])
    for t, rows in enumerate(adj):
        for i, row in enumerate(rows):
            for j in range(i + 1, n):
                if (row >> j) & 1:
                    M.add_edge(i, j, t=t)
    for a in range(pattern.Np):
        Q.add_node(a, tm=pattern.type_mask[a], cm=pattern.charge_mask[a], d=int(pattern.degree[a]),
                   h=int(pattern.min_h[a]))
        for b in range(a + 1, pattern.Np):
            if pattern.bond_mask[a, b].any():
                Q.add_edge(a, b, types=set(np.flatnonzero(pattern.bond_mask[a, b]).tolist()))

    def node_match(m, q):
        return ((not q["tm"].any() or q["tm"][m["a"]]) and (not q["cm"].any() or q["cm"][m["c"]])
                and (q["d"] < 0 or m["d"] == q["d"]) and (q["h"] < 0 or m["h"] >= q["h"]))

    gm = isomorphism.GraphMatcher(M, Q, node_match=node_match, edge_match=lambda m, q: m["t"] in q["types"])
    anchors = 0
    for mapping in gm.subgraph_monomorphisms_iter():          # molecule atom -> pattern atom
        for i, a in mapping.items():
            if a == 0:
                anchors |= 1 << i
    return anchors


def is_match(pattern, state, first):
    """Whether ``first`` (images by pattern atom) is a match, checked from the definition."""
    n, atype, charge, degree, h, adj = state
    if len(set(first)) != pattern.Np or not all(0 <= i < n for i in first):
        return False
    for a, i in enumerate(first):
        tm, cm = pattern.type_mask[a], pattern.charge_mask[a]
        if (tm.any() and not tm[atype[i]]) or (cm.any() and not cm[charge[i]]):
            return False
        if (pattern.degree[a] >= 0 and degree[i] != pattern.degree[a]) or (pattern.min_h[a] >= 0 and h[i] < pattern.min_h[a]):
            return False
        for b, j in enumerate(first):
            types = np.flatnonzero(pattern.bond_mask[a, b])
            if len(types) and not any((adj[t][i] >> j) & 1 for t in types):
                return False
    return True


def dodecahedrane():
    """(nodes, edges, n, rules name, the relaxed pattern of 10 carbons ending in N): no match, an exhaustive search."""
    r = model_rules("gdb13")
    nodes, edges = VM.molecule(20, r, [("C", 0)] * 20, [(i, j, 1) for i, j in nx.dodecahedral_graph().edges()])
    chain = VM.molecule(11, r, [("C", 0)] * 10 + [("N", 0)], [(i, i + 1, 1) for i in range(10)])
    return nodes, edges, 20, "gdb13", SM.from_molecule(*chain, 11, r, relax_bonds=True)


#: the model's own step counts on the dodecahedrane case (every anchor is equivalent: the graph is vertex-transitive,
#: but the candidate ORDER is not, so the counts are recorded per anchor from the model and asserted as constants)
DODECAHEDRANE_STEPS_DEFAULT = 957


def hand_rules():
    return model_rules("chem")


def hand_mol(symbols_charges, bonds, N=12):
    return VM.molecule(N, hand_rules(), symbols_charges, bonds)


def hand_match(pattern, mol, **kw):
    status, state = SM.molecule_state(*mol, None, hand_rules())
    assert status == 0
    m, cnt, anchors, first, lim = SM.match_one(pattern, state, **kw)
    assert m == (cnt > 0) and cnt == bin(anchors).count("1") and (first is None) == (m == 0)
    assert anchors == nx_anchors(pattern, state)
    return {i for i in range(state[0]) if (anchors >> i) & 1}, first, lim


NAPHTHALENE_BONDS = [(i, (i + 1) % 10) for i in range(10)] + [(4, 9)]    # the perimeter and the fusion bond
NAPHTHALENE_CENTRAL = {(0, 1), (2, 3), (4, 9), (5, 6), (7, 8)}            # the phase with the double bond in the middle
NAPHTHALENE_OUTER = {(1, 2), (3, 4), (5, 6), (7, 8), (9, 0)}              # one of the two others


def naphthalene(doubles):
    return hand_mol([("C", 0)] * 10, [(i, j, 2 if (i, j) in doubles else 1) for i, j in NAPHTHALENE_BONDS])


# ---- hand cases -----------------------------------------------------------------------------------------------------

def test_hand_cases_with_written_out_answers():
    r = hand_rules()
    pat = lambda atoms, bonds, **kw: SM.from_molecule(*hand_mol(atoms, bonds), len(atoms), r, **kw)
    C, N, O = ("C", 0), ("N", 0), ("O", 0)
    acetamide = hand_mol([C, C, O, N], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])
    amide = pat([C, O, N], [(0, 1, 2), (0, 2, 1)])
    assert hand_match(amide, acetamide) == ({1}, [1, 2, 3], 0)
    kekule = [(i, (i + 1) % 6, 2 - i % 2) for i in range(6)]
    toluene = hand_mol([C] * 7, kekule + [(0, 6, 1)])
    benzene = pat([C] * 6, kekule)
    anchors, first, _ = hand_match(benzene, toluene)
    assert anchors == {0, 1, 2, 3, 4, 5} and first == [0, 1, 2, 3, 4, 5]
    # a Kekule pattern against the other Kekule phase: no aromaticity is perceived
    central, outer = naphthalene(NAPHTHALENE_CENTRAL), naphthalene(NAPHTHALENE_OUTER)
    exact = SM.from_molecule(*central, 10, r)
    relaxed = SM.from_molecule(*central, 10, r, relax_bonds=True)
    assert hand_match(exact, central)[0] == {0, 3, 5, 8} and hand_match(exact, outer) == (set(), None, 0)
    assert hand_match(relaxed, outer)[0] == {0, 3, 5, 8}
    # charges
    nitromethane = hand_mol([C, ("N", 1), O, ("O", -1)], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])
    neutral = hand_mol([C, N, O, O], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])
    nitro = pat([("N", 1), O, ("O", -1)], [(0, 1, 2), (0, 2, 1)])
    nitro_any = pat([("N", 1), O, ("O", -1)], [(0, 1, 2), (0, 2, 1)], any_charge=True)
    assert hand_match(nitro, nitromethane) == ({1}, [1, 2, 3], 0) and hand_match(nitro, neutral)[0] == set()
    assert hand_match(nitro_any, nitromethane)[0] == {1} and hand_match(nitro_any, neutral) == ({1}, [1, 2, 3], 0)
    # hydrogens: C(=O)O with at least one H on the second O
    acid = hand_mol([C, C, O, O], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])
    ester = hand_mol([C, C, O, O, C], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)])
    carboxyl = pat([C, O, O], [(0, 1, 2), (0, 2, 1)])
    oh = SM.Pattern(carboxyl.type_mask, carboxyl.charge_mask, carboxyl.bond_mask, min_h=[-1, -1, 1])
    assert hand_match(carboxyl, acid)[0] == hand_match(carboxyl, ester)[0] == {1}
    assert hand_match(oh, acid) == ({1}, [1, 2, 3], 0) and hand_match(oh, ester) == (set(), None, 0)
    # degree
    propane = hand_mol([C] * 3, [(0, 1, 1), (1, 2, 1)])
    one = lambda **kw: SM.Pattern(carboxyl.type_mask[:1], carboxyl.charge_mask[:1], np.zeros((1, 1, 3)), **kw)
    assert hand_match(one(degree=[1]), propane)[0] == {0, 2} and hand_match(one(degree=[2]), propane)[0] == {1}
    assert hand_match(one(degree=[3]), propane) == (set(), None, 0)
    # a pattern larger than the molecule, Np = 1, a list of types
    decane = pat([C] * 10, [(i, i + 1, 1) for i in range(9)])
    assert hand_match(decane, propane) == (set(), None, 0)
    assert hand_match(one(), acetamide) == ({0, 1}, [0], 0)
    n_or_o = np.zeros((1, 7))
    n_or_o[0, [1, 2]] = 1
    assert hand_match(SM.Pattern(n_or_o, np.zeros((1, 3)), np.zeros((1, 1, 3))), acetamide) == ({2, 3}, [2], 0)
    # a monomorphism, not an induced subgraph: the open chain is in the ring
    ring3 = hand_mol([C] * 3, [(0, 1, 1), (1, 2, 1), (0, 2, 1)])
    assert hand_match(pat([C] * 3, [(0, 1, 1), (1, 2, 1)]), ring3)[0] == {0, 1, 2}


def test_plan_is_breadth_first_with_back_bonds():
    # atom 0 - {2, 3}, 2 - 1, 3 - 1, 1 - 4, 4 - 0: order 0 2 3 4 1; 1 is discovered from 2, its back bonds go to 3 and 4
    bonded = np.zeros((5, 5), bool)
    for a, b in ((0, 2), (0, 3), (2, 1), (3, 1), (1, 4), (4, 0)):
        bonded[a, b] = bonded[b, a] = True
    assert SM.plan(bonded) == ([0, 2, 3, 4, 1], [0, 0, 0, 0, 1], [[], [], [], [], [2, 3]])
    bonded[0, 3] = bonded[3, 0] = bonded[3, 1] = bonded[1, 3] = False
    with pytest.raises(ValueError, match="not connected"):
        SM.plan(bonded)
    assert SM.plan(np.zeros((1, 1), bool)) == ([0], [0], [[]])


# ---- against networkx -----------------------------------------------------------------------------------------------

def test_drd2_molecules_against_networkx_and_the_step_limit_never_fires(golden_dir):
    states = drd2_states(golden_dir)
    assert len(states) == 863 and all(s is not None for s in states)
    worst, found = 0, np.zeros((2, len(PATTERNS18)), int)
    for relax in (False, True):
        for pi, pattern in enumerate(drd2_patterns(relax)):
            for g, state in enumerate(states):
                steps = []
                m, cnt, anchors, first, lim = SM.match_one(pattern, state, steps_out=steps)
                assert lim == 0, (relax, pi, g)                # the default cap never fires on the fixtures
                worst = max([worst] + [s for _, s in steps])
                found[int(relax), pi] += m
                if g < 150:
                    assert anchors == nx_anchors(pattern, state), (relax, list(PATTERNS18)[pi], g)
                if m:                                          # first: a match, from the lowest anchor
                    assert is_match(pattern, state, first) and first[0] == (anchors & -anchors).bit_length() - 1
    print(f"\nworst anchor: {worst} steps; molecules matched, exact: {found[0].tolist()}, relaxed: {found[1].tolist()}")
    assert worst == 112
    assert (found > 0).all() and (found[1] >= found[0]).all() and found[0, 16] == 863
    assert found[1, 4] > found[0, 4] and found[1, 0] > found[0, 0]       # Kekule phases: relaxing finds more


@pytest.mark.parametrize("c", STORED_SETS)
def test_stored_sets_against_networkx(golden_dir, c):
    nodes, edges, n, _ = stored_set(golden_dir, c)
    r, pats = model_rules(c), set_patterns(c)
    hits = {name: 0 for name in pats}
    for g in range(len(nodes)):
        status, state = SM.molecule_state(nodes[g], edges[g], None if n is None else n[g], r)
        if state is None:
            continue
        for name, pattern in pats.items():
            m, cnt, anchors, first, lim = SM.match_one(pattern, state)
            assert anchors == nx_anchors(pattern, state) and lim == 0, (c, name, g)
            assert not m or (is_match(pattern, state, first) and first[0] == (anchors & -anchors).bit_length() - 1)
            hits[name] += m
    print(c, hits)
    assert hits["any_any"] > 0 and hits["N_or_O"] >= hits["N_or_O_with_H"] > 0       # there is something to find
    assert c != "gdb13" or all(v > 0 for v in hits.values())


def test_anchors_move_with_the_atoms_under_8_node_orders(golden_dir):
    nodes, edges, n = drd2_molecules(golden_dir)
    rng = np.random.default_rng(8)
    r = drd2_rules()
    for g in (0, 7, 100, 500):
        k = int(n[g])
        base = SM.molecule_state(nodes[g], edges[g], None, r)[1]
        for _ in range(8):
            perm = np.concatenate([rng.permutation(k), np.arange(k, nodes.shape[1])])      # new atom i is old perm[i]
            state = SM.molecule_state(nodes[g][perm], edges[g][perm][:, perm], None, r)[1]
            for relax in (False, True):
                for pattern in drd2_patterns(relax):
                    old = SM.match_one(pattern, base)[2]
                    new = SM.match_one(pattern, state)[2]
                    assert new == sum(1 << i for i in range(k) if (old >> int(perm[i])) & 1)


# ---- the limit ------------------------------------------------------------------------------------------------------

def test_the_step_limit_on_an_exhaustive_search():
    nodes, edges, n, c, pattern = dodecahedrane()
    r = model_rules(c)
    state = SM.molecule_state(nodes, edges, n, r)[1]
    assert nx_anchors(pattern, state) == 0
    steps = []
    assert SM.match_one(pattern, state, steps_out=steps) == (0, 0, 0, None, 0)
    assert [a for a, _ in steps] == list(range(20)) and {s for _, s in steps} == {DODECAHEDRANE_STEPS_DEFAULT}
    steps = []
    assert SM.match_one(pattern, state, max_steps=64, steps_out=steps) == (0, 0, 0, None, 20)
    assert [s for _, s in steps] == [64] * 20
    assert SM.match_one(pattern, state, max_steps=DODECAHEDRANE_STEPS_DEFAULT)[4] == 0       # exactly enough
    assert SM.match_one(pattern, state, max_steps=DODECAHEDRANE_STEPS_DEFAULT - 1)[4] == 20
    full = SM.substructure(nodes[None], edges[None], np.array([n]), r, [pattern], max_steps=64)
    assert full["status"].tolist() == [SM.SUB_STEP_LIMIT] and full["n_limited"].tolist() == [[20]]
    assert full["match"].tolist() == [[0]] and (full["first"] == -1).all()
    assert SM.substructure(nodes[None], edges[None], np.array([n]), r, [pattern])["status"].tolist() == [0]


def test_batch_model_status_and_pattern_index():
    from tests.test_valence_cpu import status_cases
    cases = status_cases()
    r = model_rules("gdb13")
    pats = [set_patterns("gdb13")[k] for k in ("CC", "any_any", "N_or_O")]
    nodes, edges = np.stack([c[0] for c in cases.values()]), np.stack([c[1] for c in cases.values()])
    n = np.array([c[2] for c in cases.values()])
    res = SM.substructure(nodes, edges, n, r, pats)
    for g, (name, case) in enumerate(cases.items()):
        assert res["status"][g] == case[3] & SM.LABEL_BITS, name
        if res["status"][g]:
            assert not res["match"][g].any() and (res["first"][g] == -1).all() and not res["anchors"][g].any()
    assert res["match"][list(cases).index("sound")].tolist() == [0, 1, 1]
    over = list(cases).index("over")                                                  # valence is not its business
    assert res["match"][over].tolist() == [0, 1, 1] and res["status"][over] == 0 and res["n_anchors"][over, 1] == 3
    idx = np.arange(len(cases)) % 5 - 1                                               # -1 and 3 are out of range
    one = SM.substructure(nodes, edges, n, r, pats, pattern_index=idx)
    for g in range(len(cases)):
        if 0 <= idx[g] < 3:
            assert one["status"][g] == res["status"][g]
            for k in ("match", "n_anchors", "n_limited", "anchors", "first"):
                assert np.array_equal(one[k][g, 0], res[k][g, idx[g]])
        else:
            assert one["status"][g] == res["status"][g] | SM.SUB_PATTERN_INDEX and not one["match"][g].any()
    assert SM.score(res["match"], require=[1], forbid=[0]).tolist() == \
        [float(m[1] and not m[0]) for m in res["match"].tolist()]


# ---- the library's host side ------------------------------------------------------------------------------------------

def decode_table(ps):
    """The packed table of a SubstructureSet back into per-pattern (Np, order, parent, parent masks, back [(q, mask)],
    degree, min_h, type words, charge words)."""
    t = ps.table
    P, Npm, A, C, Fe, TW, CW, B = t[:8].tolist()
    R = 8 + -(-(TW + CW) // 4) * 4
    S = 4 + Npm * R + B
    assert len(t) == 8 + P * S and B % 4 == 0
    out = []
    for p in range(P):
        rec = t[8 + p * S:8 + (p + 1) * S]
        Np = int(rec[0])
        rows = [rec[4 + k * R:4 + (k + 1) * R] for k in range(Np)]
        back = [[(int(e) & 0xff, int(e) >> 8) for e in rec[4 + Npm * R + row[2]:4 + Npm * R + row[2] + row[3]]]
                for row in rows]
        out.append(dict(Np=Np, order=[int(row[4]) for row in rows], parent=[int(row[0]) for row in rows],
                        pmask=[int(row[1]) for row in rows], back=back, degree=[int(row[5]) for row in rows],
                        min_h=[int(row[6]) for row in rows], tw=[row[8:8 + TW].tolist() for row in rows],
                        cw=[row[8 + TW:8 + TW + CW].tolist() for row in rows]))
    return out


def check_set_against_model(ps, patterns):
    word = lambda row: sum(1 << int(t) for t in np.flatnonzero(row))
    full = lambda row: word(row) if row.any() else (1 << len(row)) - 1
    assert len(ps) == len(patterns) and ps.n_atoms == [p.Np for p in patterns]
    for got, p, order, parent, back in zip(decode_table(ps), patterns, ps.order, ps.parent, ps.back):
        assert (order, parent, back) == (p.order, p.parent, p.back)                   # the plan: library == model
        assert (got["Np"], got["order"], got["parent"]) == (p.Np, p.order, p.parent)
        for k, a in enumerate(p.order):
            assert got["pmask"][k] == (word(p.bond_mask[a, p.order[p.parent[k]]]) if k else 0)
            assert got["back"][k] == [(q, word(p.bond_mask[a, p.order[q]])) for q in p.back[k]]
            assert (got["degree"][k], got["min_h"][k]) == (p.degree[a], p.min_h[a])
            assert got["tw"][k] == [full(p.type_mask[a])] and got["cw"][k] == [full(p.charge_mask[a])]


def test_the_packed_plan_equals_the_models():
    for relax in (False, True):
        pats = drd2_patterns(relax)
        ps = analyze.SubstructureSet(**stack_patterns(pats), names=list(PATTERNS18), device=None)
        check_set_against_model(ps, pats)
        assert ps.Np_max == 12 and ps.dims == (7, 3, 3) and ps.index("amide") == 1 and ps.index(3) == 3
        nodes, edges, n = pattern_molecules()
        same = analyze.SubstructureSet.from_molecules(nodes, edges, n, analyze.ValenceRules(device=None, **DRD2_ARGS),
                                                      relax_bonds=relax, device=None)
        assert np.array_equal(same.table, ps.table)
    for c in STORED_SETS:
        pats = list(set_patterns(c).values())
        check_set_against_model(analyze.SubstructureSet(**stack_patterns(pats), device=None), pats)
    naph = decode_table(analyze.SubstructureSet(**stack_patterns(drd2_patterns(False)[4:5]), device=None))[0]
    assert sum(len(b) for b in naph["back"]) == 2                                     # two rings: two ring-closing bonds


def test_pattern_set_value_errors():
    ok = stack_patterns(drd2_patterns(False)[:3])
    new = lambda **kw: analyze.SubstructureSet(**{**ok, **kw}, device=None)
    split = ok["bond_mask"].copy()
    split[2, 0, 1] = split[2, 1, 0] = split[2, 0, 5] = split[2, 5, 0] = 0             # piperazine without atom 0's bonds
    with pytest.raises(ValueError, match="not connected"):
        new(bond_mask=split)
    with pytest.raises(ValueError, match="not connected"):                             # a predicate on a loose atom
        new(degree=np.where(np.arange(6)[None, :] == 5, 2, -1).repeat(3, axis=0))
    one_way = ok["bond_mask"].copy()
    one_way[0, 0, 1] = 0
    with pytest.raises(ValueError, match="symmetric"):
        new(bond_mask=one_way)
    loop = ok["bond_mask"].copy()
    loop[0, 1, 1, 0] = 1
    with pytest.raises(ValueError, match="bonded to itself"):
        new(bond_mask=loop)
    with pytest.raises(ValueError, match="at least one pattern"):
        new(type_mask=ok["type_mask"][:0], charge_mask=ok["charge_mask"][:0], bond_mask=ok["bond_mask"][:0])
    with pytest.raises(ValueError, match="do not match"):
        new(charge_mask=ok["charge_mask"][:, :5])
    with pytest.raises(ValueError, match="3-dimensional"):
        new(type_mask=ok["type_mask"][0])
    with pytest.raises(ValueError, match="at most 32 atoms"):
        analyze.SubstructureSet(np.zeros((1, 33, 7)), np.zeros((1, 33, 3)), np.zeros((1, 33, 33, 3)), device=None)
    with pytest.raises(ValueError, match="degree must be integers"):
        new(degree=np.full((3, 6), 128))
    with pytest.raises(ValueError, match="min_h must be integers"):
        new(min_h=np.full((3, 6), -2))
    with pytest.raises(ValueError, match="names"):
        new(names=["a", "a", "b"])
    with pytest.raises(ValueError, match="no pattern named"):
        new(names=["a", "b", "c"]).index("d")
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.SubstructureSet(**ok, device="cpu")
    rules = analyze.ValenceRules(device=None, **DRD2_ARGS)
    nodes, edges, n = pattern_molecules()
    with pytest.raises(ValueError, match="1 to 32 atoms"):
        analyze.SubstructureSet.from_molecules(nodes, edges, n * 0, rules, device=None)
    with pytest.raises(ValueError, match="not one-hot"):
        analyze.SubstructureSet.from_molecules(nodes * 0, edges, n, rules, device=None)
    with pytest.raises(TypeError, match="ValenceRules"):
        analyze.SubstructureSet.from_molecules(nodes, edges, n, None, device=None)
    loose = nodes[:1].copy()
    loose[0, 6:12] = loose[0, :6]                                          # benzene and six atoms without a bond
    with pytest.raises(ValueError, match="not connected"):
        analyze.SubstructureSet.from_molecules(loose, edges[:1], None, rules, device=None)


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    decl = re.search(r"^int\s+gi_mol_substructure\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert "gi_mol_substructure" in L.SIGNATURES and hasattr(lib, "gi_mol_substructure")
    assert len(L.SIGNATURES["gi_mol_substructure"][1]) == len(decl.split(",")) == 26
    for name, value in (("MAX_ATOMS", "32"), ("MAX_PATTERNS", "65536"), ("MAX_STEPS", r"\(1 << 20\)"),
                        ("STEP_LIMIT", r"\(1 << 21\)"), ("PATTERN_INDEX", r"\(1 << 22\)")):
        assert re.search(rf"#define\s+GI_SUB_{name}\s+{value}", hdr), name
    assert (L.SUB_MAX_ATOMS, L.SUB_MAX_PATTERNS, L.SUB_MAX_STEPS) == (32, 65536, 1 << 20) == \
        (SM.MAX_PATTERN_ATOMS, 65536, SM.MAX_STEPS_LIMIT)
    assert (L.SUB_STEP_LIMIT, L.SUB_PATTERN_INDEX) == (SM.SUB_STEP_LIMIT, SM.SUB_PATTERN_INDEX) == (1 << 21, 1 << 22)
    assert SM.LABEL_BITS == analyze.MALFORMED_BITS | L.VAL_EMPTY | L.VAL_SELF_LOOP
    assert set(analyze.SUBSTRUCTURE_STATUS_MESSAGES) == {1, 2, 8, 16, 32, 64, 128, 256, 1 << 21, 1 << 22}
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # an added entry point is compatible
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_substructure.hip")).read()
    assert "gi_substructure.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    assert "getenv" not in src and "atomicAdd" not in src and "gi_read_labelled<true>" in src
    assert "gi_mol_substructure" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # argument checks that need no device: nothing is launched for any of these
    ps = analyze.SubstructureSet(**stack_patterns(drd2_patterns(False)), device=None)

    def call(G=0, N=72, Fn=14, Fe=3, dtype=1, nb=1, A=7, C=3, H=4, table=ps.table, words=None, steps=4096):
        return lib.gi_mol_substructure(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, None,
                                       None if table is None else table.ctypes.data, None,
                                       (0 if table is None else table.size) if words is None else words, None, steps,
                                       None, None, None, None, None, None, None)
    assert call() == 0 and call(table=None) == 0                           # an empty batch: no launch
    assert call(G=1) == -1                                                 # no buffers
    assert call(N=129) == -1 and call(Fe=9) == -1 and call(G=-1) == -1 and call(Fn=513) == -2
    assert call(dtype=2) == -1 and call(nb=2) == -1 and call(A=8, C=3, H=4) == -1
    assert call(steps=0) == -1 and call(steps=(1 << 20) + 1) == -2 and call(steps=1 << 20) == 0
    assert call(Fe=2) == -1 and call(A=6, C=3) == -1 and call(words=ps.table.size - 1) == -1 and call(words=4) == -1

    def broken(offset, value):
        t = ps.table.copy()
        t[offset] = value
        return call(table=t)
    R = 12
    row = lambda k: 8 + 4 + k * R                                          # of pattern 0, benzene
    assert broken(0, 0) == -1 and broken(0, 65537) in (-1, -2) and broken(1, 33) == -2 and broken(7, 3) == -1
    assert broken(8, 0) == -1 and broken(8, 13) == -1                      # Np
    assert broken(row(1), 1) == -1 and broken(row(1), -1) == -1            # a parent that is not earlier
    assert broken(row(0), 1) == -1 and broken(row(2) + 1, 0) == -1 and broken(row(2) + 1, 8) == -1
    assert broken(row(2) + 4, 0) == -1 and broken(row(2) + 4, 6) == -1     # the plan is not a permutation / out of range
    assert broken(row(5) + 2, -1) == -1 and broken(row(5) + 3, 5) == -1    # back bonds outside the record's list
    assert broken(row(3) + 5, 128) == -1 and broken(row(3) + 6, 16) == -1 and broken(row(3) + 8, 1 << 7) == -1
    benzene = decode_table(ps)[0]                           # order 0 1 5 2 4 3: the ring closes from position 5 to 4
    assert benzene["order"] == [0, 1, 5, 2, 4, 3] and benzene["parent"][5] == 3 and benzene["back"][5][0][0] == 4
    back0 = 8 + 4 + 12 * R                                  # a back bond to itself, without types, to its parent
    assert broken(back0, 5 | (1 << 8)) == -1 and broken(back0, 4) == -1 and broken(back0, 3 | (1 << 8)) == -1
    assert broken(back0, 4 | (8 << 8)) == -1 and broken(back0, 4 | (3 << 8)) == 0


def test_python_boundary_raises():
    n, e = torch.zeros(2, 72, 14, dtype=torch.int8), torch.zeros(2, 72, 72, 3, dtype=torch.int8)
    host_rules = analyze.ValenceRules(device=None, **DRD2_ARGS)
    host_set = analyze.SubstructureSet(**stack_patterns(drd2_patterns(False)), device=None)
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.substructure(n, e, None, host_rules, host_set)
    with pytest.raises(TypeError, match="tensor"):
        analyze.substructure(n.numpy(), e.numpy(), None, host_rules, host_set)
    with pytest.raises(TypeError, match="ValenceRules"):
        analyze.substructure(n, e, None, [7, 3], host_set)
    with pytest.raises(TypeError, match="SubstructureSet"):
        analyze.substructure(n, e, None, host_rules, [host_set])
    for bad in (0, (1 << 20) + 1, 4096.0, True):
        with pytest.raises(ValueError, match="max_steps"):
            analyze.substructure(n, e, None, host_rules, host_set, max_steps=bad)
    with pytest.raises(TypeError, match="substructure's result"):
        analyze.substructure_score(n)
    res = analyze.SubstructureMatches(torch.zeros(analyze.SubstructureMatches.nbytes(2, 18, 12), dtype=torch.uint8), 2, 18,
                                      12, patterns=host_set)
    res.match[0, [1, 3]] = 1
    res.match[1, [1, 2, 3]] = 1
    assert analyze.substructure_score(res, require=[1, 3], forbid=[0, 2]).tolist() == [1.0, 0.0]
    assert analyze.substructure_score(res, require=[3, 1, 2]).tolist() == [0.0, 1.0]
    assert analyze.substructure_score(res).tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="not an index"):
        analyze.substructure_score(res, require=[18])
    assert analyze.SubstructureMatches.nbytes(0, 18, 12) == 0 and analyze.SubstructureMatches.nbytes(1, 2, 3) == 4 * (1 + 6 + 8 + 6)
    if not torch.cuda.is_available():
        return
    dn, de = n.cuda(), e.cuda()                                            # raised before anything is launched
    rules, ps = analyze.ValenceRules(**DRD2_ARGS), analyze.SubstructureSet(**stack_patterns(drd2_patterns(False)))
    with pytest.raises(RuntimeError, match="device=None"):
        analyze.substructure(dn, de, None, rules, host_set)
    with pytest.raises(ValueError, match="contiguous"):
        analyze.substructure(dn, de.transpose(1, 2), None, rules, ps)
    with pytest.raises(TypeError, match="float32 or both int8"):
        analyze.substructure(dn.float(), de, None, rules, ps)
    with pytest.raises(ValueError, match="does not match"):
        analyze.substructure(dn, de[:, :71], None, rules, ps)
    with pytest.raises(ValueError, match="were built for"):
        analyze.substructure(dn, de[..., :2].contiguous(), None, analyze.ValenceRules(bond_orders=(1, 2), **DRD2_ARGS), ps)
    with pytest.raises(RuntimeError, match="pattern_index"):
        analyze.substructure(dn, de, None, rules, ps, pattern_index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="pattern_index"):
        analyze.substructure(dn, de, None, rules, ps, pattern_index=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="pattern_index"):
        analyze.substructure(dn, de, None, rules, ps, pattern_index=torch.zeros(3, dtype=torch.int32, device="cuda"))
