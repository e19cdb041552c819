"""The resonance normal form WITHOUT a device: tests/resonance_model.py (the specification of csrc/gi_resonance.hip) is
pinned to hand cases with written-out bond lists, to networkx's matchings on every bond of G' (the DRD2 fixtures, the
generated ring systems of tests/test_kekulize_cpu.py, two N = 128 cases), to phase invariance on re-drawn Kekule
structures, and to its round trips; the host-device search of csrc/gi_res_search.h is compiled for the host and run
against the model on the same inputs; the entry points' and the Python boundary's checks that need no launch."""
import os
import random
import re
import shutil
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import canon_model as CM
from tests import resonance_model as XM
from tests import smiles_model as SM
from tests import valence_model as VM
from tests.test_kekulize_cpu import DRD2_ARGS, DRD2_N, drd2_model, drd2_rules, generated_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphinvent_amd", "csrc")
_CACHE = {}

HAND_ARGS = dict(atom_types=["C", "N", "O"], formal_charge=[-1, 0, 1])
HAND_N = 13


def ring_bonds(n, first=0, double_first=True):
    """An n-ring on atoms first .. first + n - 1 with alternating orders."""
    return [(first + i, first + (i + 1) % n, 2 if (i % 2 == 0) == double_first else 1) for i in range(n)]


NAPHTHALENE = [(i, (i + 1) % 10) for i in range(10)] + [(4, 9)]               # the perimeter and the fusion bond
NAPHTHALENE_CENTRAL = {(0, 1), (2, 3), (4, 9), (5, 6), (7, 8)}
NAPHTHALENE_OUTER = {(1, 2), (3, 4), (5, 6), (7, 8), (0, 9)}


def with_doubles(pairs, doubles):
    return [(a, b, 2 if (min(a, b), max(a, b)) in doubles else 1) for a, b in pairs]


#: name -> (symbols, bonds (a, b, order), the delocalised bonds expected)
HAND = {
    "benzene": ("CCCCCC", ring_bonds(6), {(i, (i + 1) % 6) for i in range(6)}),
    "naphthalene_central": ("C" * 10, with_doubles(NAPHTHALENE, NAPHTHALENE_CENTRAL), set(NAPHTHALENE)),
    "naphthalene_outer": ("C" * 10, with_doubles(NAPHTHALENE, NAPHTHALENE_OUTER), set(NAPHTHALENE)),
    "biphenyl": ("C" * 12, ring_bonds(6) + ring_bonds(6, 6) + [(5, 6, 1)],
                 {(i, (i + 1) % 6) for i in range(6)} | {(6 + i, 6 + (i + 1) % 6) for i in range(6)}),
    "azulene": ("C" * 10, ring_bonds(10) + [(0, 6, 1)], {(i, (i + 1) % 10) for i in range(10)}),
    "indole": ("CCCCCCCCN", ring_bonds(6) + [(4, 6, 1), (6, 7, 2), (7, 8, 1), (8, 5, 1)],
               {(i, (i + 1) % 6) for i in range(6)}),
    "pyrrole": ("NCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], set()),
    "furan": ("OCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], set()),
    "butadiene": ("CCCC", [(0, 1, 2), (1, 2, 1), (2, 3, 2)], set()),
    "quinone": ("CCCCCCOO", [(0, 6, 2), (3, 7, 2), (0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 2), (5, 0, 1)], set()),
    "cyclooctatetraene": ("C" * 8, ring_bonds(8), {(i, (i + 1) % 8) for i in range(8)}),
    "cyclobutadiene": ("CCCC", ring_bonds(4), {(i, (i + 1) % 4) for i in range(4)}),
    "pentalene": ("C" * 8, ring_bonds(8) + [(0, 4, 1)], {(i, (i + 1) % 8) for i in range(8)}),
    # an allene on a ring: 7 has two double bonds, so 6 (its partner is 7) and 8 stay out of V' as well
    "allene_on_ring": ("C" * 9, ring_bonds(6) + [(0, 6, 1), (6, 7, 2), (7, 8, 2)], {(i, (i + 1) % 6) for i in range(6)}),
    # an ene-yne on a ring: 7 carries the triple bond, so 6 = 7 is outside V'
    "eneyne_on_ring": ("C" * 9, ring_bonds(6) + [(0, 6, 1), (6, 7, 2), (7, 8, 3)], {(i, (i + 1) % 6) for i in range(6)}),
    # the same chains INSIDE the ring's alternation: a ring atom with a second double bond breaks every cycle through it
    "exocyclic_double_on_ring_atom": ("C" * 7, ring_bonds(6) + [(0, 6, 2)], set()),
    "ethene": ("CC", [(0, 1, 2)], set()),
    "single_atom": ("C", [], set()),
}
OUT_OF_V = {"allene_on_ring": (6, 7, 8), "eneyne_on_ring": (6, 7, 8), "exocyclic_double_on_ring_atom": (0, 1, 6)}


def hand_rules(aromatic_type=False):
    return VM.Rules(bond_orders=(1, 2, 3, 1.5) if aromatic_type else (1, 2, 3), **HAND_ARGS)


def hand_molecule(symbols, bonds, rules, N=HAND_N):
    return VM.molecule(N, rules, [(s, 0) for s in symbols], bonds)


def hand_batch():
    """-> (names, nodes [G, 13, 6], edges [G, 13, 13, 3], n_nodes [G]) of HAND, int8."""
    rules = hand_rules()
    mols = [hand_molecule(s, b, rules) for s, b, _ in HAND.values()]
    return (list(HAND), np.stack([m[0] for m in mols]), np.stack([m[1] for m in mols]),
            np.array([len(s) for s, _, _ in HAND.values()], np.int32))


def error_inputs():
    """name -> (nodes, edges, n_given, the bit), one input per bit of the front end, on Kekule benzene at N = 13."""
    rules = hand_rules()
    out = {}

    def case(name, bit, n_given=6):
        nodes, edges = hand_molecule("CCCCCC", ring_bonds(6), rules)
        out[name] = [nodes, edges, n_given, bit]
        return nodes, edges
    nodes, _ = case("onehot", VM.MOL_ONEHOT)
    nodes[2, 1] = 1                                                         # atom 2 is C and N
    case("bond_past_n", VM.MOL_BOND_PAST_N | VM.MOL_NODE_PAST_N, n_given=5)
    _, edges = case("value", VM.MOL_VALUE)
    edges[0, 1, 1] = edges[1, 0, 1] = 2
    _, edges = case("multi_bond", VM.MOL_MULTI_BOND)
    edges[0, 1, 0] = edges[1, 0, 0] = 1
    _, edges = case("asymmetric", VM.MOL_ASYMMETRIC)
    edges[1, 0, 1] = 0
    nodes, _ = case("node_past_n", VM.MOL_NODE_PAST_N)
    nodes[7, 0] = 1                                                         # a set entry in a row past n
    nodes, edges = case("empty", XM.RES_EMPTY, n_given=0)
    nodes[:], edges[:] = 0, 0
    _, edges = case("self_loop", XM.RES_SELF_LOOP)
    edges[3, 3, 0] = 1
    return out


def ring128():
    rules = drd2_rules()
    return VM.molecule(128, rules, [("C", 0, 1)] * 128, ring_bonds(128))


def polyacene128():
    """A ladder of 64 + 64 atoms with a rung at every second position (the polyacene's rings) and one at the far end:
    159 bonds in G'; the double bonds are a perfect matching networkx draws."""
    rules = drd2_rules()
    pairs = [(i, i + 1) for i in range(63)] + [(64 + i, 65 + i) for i in range(63)] + \
            [(i, 64 + i) for i in range(0, 64, 2)] + [(63, 127)]
    g = nx.Graph(pairs)
    m = nx.max_weight_matching(g, maxcardinality=True)
    assert len(m) == 64
    doubles = {(min(a, b), max(a, b)) for a, b in m}
    deg = [g.degree(i) for i in range(128)]
    atoms = [("C", 0, 4 - deg[i] - 1) for i in range(128)]
    return VM.molecule(128, rules, atoms, with_doubles(pairs, doubles))


def big_batch():
    """The two N = 128 cases -> (nodes, edges, n_nodes)."""
    if "big" not in _CACHE:
        mols = [ring128(), polyacene128()]
        _CACHE["big"] = np.stack([m[0] for m in mols]), np.stack([m[1] for m in mols]), np.array([128, 128], np.int32)
    return _CACHE["big"]


def model_of(name, golden_dir=None):
    """-> (inputs dict(nodes, edges, n_nodes), rules, the model's result, its traces), computed once and shared."""
    key = "model_" + name
    if key not in _CACHE:
        if name == "hand":
            _, nodes, edges, n = hand_batch()
            rules = hand_rules()
        elif name == "drd2":
            out = drd2_model(golden_dir)[0]
            nodes, edges, n, rules = out["nodes"], out["edges"], out["n_nodes"], drd2_rules()
        elif name == "generated":
            out = generated_model()[0]
            nodes, edges, n, rules = out["nodes"], out["edges"], out["n_nodes"], drd2_rules()
        else:
            nodes, edges, n = big_batch()
            rules = drd2_rules()
        traces = []
        res = XM.resonance(nodes, edges, n, rules, traces)
        _CACHE[key] = dict(nodes=nodes, edges=edges, n_nodes=n), rules, res, traces
    return _CACHE[key]


def rephase(edges, trace, rules, rng):
    """The molecule with its double bonds inside V' redrawn as another perfect matching of G' (random weights)."""
    g = nx.Graph()
    for (a, b) in trace["order"]:
        if a < b:
            g.add_edge(a, b, weight=rng.random())
    m = nx.max_weight_matching(g, maxcardinality=True)
    assert 2 * len(m) == g.number_of_nodes()
    doubles = {(min(a, b), max(a, b)) for a, b in m}
    out = edges.copy()
    t1, t2 = rules.order2.index(2), rules.order2.index(4)
    for (a, b) in trace["order"]:
        out[a, b] = 0
        out[a, b, t2 if (min(a, b), max(a, b)) in doubles else t1] = 1
    return out


def rephased_drd2(golden_dir):
    """-> (edges [863, 72, 72, 3] re-phased with a fixed seed, the indices whose stored phase changed)."""
    if "rephased" not in _CACHE:
        inp, rules, _, traces = model_of("drd2", golden_dir)
        rng = random.Random(20261021)
        edges = np.stack([rephase(inp["edges"][g], traces[g], rules, rng) for g in range(len(traces))])
        changed = [g for g in range(len(traces)) if not np.array_equal(edges[g], inp["edges"][g])]
        _CACHE["rephased"] = edges, changed
    return _CACHE["rephased"]


def bonds_in(rows, N):
    """The 128-bit rows [N, 4] int32 -> {(a, b)}, a < b."""
    rows = np.asarray(rows).view(np.uint32)
    return {(a, b) for a in range(N) for b in range(a + 1, N) if (rows[a, b >> 5] >> (b & 31)) & 1}


def test_hand_cases_with_written_out_answers():
    names, nodes, edges, n = hand_batch()
    inp, rules, res, traces = model_of("hand")
    counts = dict(benzene=6, naphthalene_central=11, naphthalene_outer=11, biphenyl=12, azulene=10, indole=6, pyrrole=0,
                  furan=0, butadiene=0, quinone=0, cyclooctatetraene=8, cyclobutadiene=4, pentalene=8)
    for g, name in enumerate(names):
        want = {(min(a, b), max(a, b)) for a, b in HAND[name][2]}
        assert bonds_in(res["delocalized"][g], HAND_N) == want, name
        assert res["n_delocalized"][g] == len(want) == counts.get(name, len(want)) and res["status"][g] == 0, name
        assert res["n_atoms"][g] == len({a for p in want for a in p}), name
        for a, b in want:                                                   # channel Fe and no other, both ways
            assert res["edges"][g, a, b].tolist() == [0, 0, 0, 1] == res["edges"][g, b, a].tolist(), name
        rest = res["edges"][g].copy()
        for a, b in want:
            rest[a, b] = rest[b, a] = 0
        stored = edges[g].copy()
        for a, b in want:
            stored[a, b] = stored[b, a] = 0
        assert np.array_equal(rest[:, :, :3], stored) and not rest[:, :, 3].any(), name       # every other bond as stored
        for i in OUT_OF_V.get(name, ()):
            assert not traces[g]["in_v"][i], (name, i)
    by = dict(zip(names, range(len(names))))
    assert res["n_systems"][by["biphenyl"]] == 2 and res["n_systems"][by["naphthalene_outer"]] == 1
    assert res["n_systems"][by["pyrrole"]] == 0 and res["n_systems"][by["benzene"]] == 1
    assert (5, 6) not in bonds_in(res["delocalized"][by["biphenyl"]], HAND_N)              # the linker
    assert (0, 6) not in bonds_in(res["delocalized"][by["azulene"]], HAND_N)               # the fusion bond
    assert np.array_equal(res["edges"][by["naphthalene_central"]], res["edges"][by["naphthalene_outer"]])
    assert not np.array_equal(edges[by["naphthalene_central"]], edges[by["naphthalene_outer"]])


def test_a_stored_aromatic_bond_sets_the_bit_and_changes_nothing():
    rules = hand_rules(aromatic_type=True)
    nodes, edges = hand_molecule("CCCCCC", [(i, (i + 1) % 6, 1.5) for i in range(6)], rules)
    one = XM.resonance_one(nodes, edges, 6, rules)
    assert one["status"] == XM.RES_AROMATIC and one["n_delocalized"] == 0 and not one["delocalized"].any()
    assert np.array_equal(one["edges"][:, :, :4], edges) and not one["edges"][:, :, 4].any()
    # Kekule benzene whose atom 0 also carries a 1.5 bond: 0 and its partner 1 leave V', no cycle is left
    nodes, edges = hand_molecule("CCCCCCC", ring_bonds(6) + [(0, 6, 1.5)], rules)
    trace = {}
    one = XM.resonance_one(nodes, edges, 7, rules, trace)
    assert one["status"] == XM.RES_AROMATIC and one["n_delocalized"] == 0 and trace["in_v"][:3] == [False, False, True]
    # ... and with the 1.5 bond away from the ring the ring is found
    nodes, edges = hand_molecule("CCCCCCCC", ring_bonds(6) + [(0, 6, 1), (6, 7, 1.5)], rules)
    one = XM.resonance_one(nodes, edges, 8, rules)
    assert one["status"] == XM.RES_AROMATIC and one["n_delocalized"] == 6 and one["edges"][6, 7].tolist() == [0, 0, 0, 1, 0]


def test_one_input_per_error_bit():
    rules = hand_rules()
    for name, (nodes, edges, n_given, bit) in error_inputs().items():
        one = XM.resonance_one(nodes, edges, n_given, rules)
        assert one["status"] == bit, (name, one["status"])
        assert one["n_delocalized"] == one["n_atoms"] == one["n_systems"] == 0 and not one["delocalized"].any(), name
        as_stored = (edges != 0) * (2 if bit & VM.MOL_VALUE else 1)         # 2 throughout: MOL_VALUE stays visible
        assert np.array_equal(one["edges"][:, :, :3], as_stored) and not one["edges"][:, :, 3].any(), name
        # ``canonical`` says about the normal form what it says about the stored molecule
        assert CM.status_of(nodes, one["edges"], n_given)[0] == CM.status_of(nodes, edges, n_given)[0], name
        k = XM.kekulize_one(nodes, one["edges"], n_given, rules)
        assert k["status"] == bit and not k["edges"].any(), name
    # kekulize's own bits: three atoms in a row have no perfect matching; rules without a double type
    nodes, edges = hand_molecule("CCC", [], rules)
    marked = np.concatenate([edges, np.zeros((HAND_N, HAND_N, 1), np.int8)], axis=2)
    marked[0, 1, 3] = marked[1, 0, 3] = marked[1, 2, 3] = marked[2, 1, 3] = 1
    k = XM.kekulize_one(nodes, marked, 3, rules)
    assert k["status"] == XM.RES_NO_KEKULE and not k["edges"].any()
    no_double = VM.Rules(bond_orders=(1, 3), **HAND_ARGS)
    marked2 = np.zeros((HAND_N, HAND_N, 3), np.int8)
    marked2[0, 1, 2] = marked2[1, 0, 2] = 1
    k = XM.kekulize_one(nodes, marked2, 3, no_double)
    assert k["status"] == XM.RES_BOND_ORDER and not k["edges"].any()
    marked2[:] = 0
    marked2[0, 1, 0] = marked2[1, 0, 0] = 1                                 # no channel-Fe bond: no type is needed
    k = XM.kekulize_one(nodes, marked2, 3, no_double)
    assert k["status"] == 0 and np.array_equal(k["edges"], marked2[:, :, :2])


def nx_verdicts(trace):
    """{(a, b)}, a < b: the bonds of G' whose reduced graph has a perfect matching by networkx.  The reduced graph is
    cut to the component of G' that holds the bond: every other component keeps its own double bonds as a perfect
    matching, so the whole reduced graph has one iff that component's part has."""
    g = nx.Graph((a, b) for (a, b) in trace["order"] if a < b)
    out = set()
    for comp in nx.connected_components(g):
        sub = g.subgraph(comp)
        for a, b in sub.edges():
            h = nx.Graph(sub)
            if trace["order"][(a, b)] == 2:
                h.remove_edge(a, b)
            else:
                h.remove_nodes_from((a, b))
            if 2 * len(nx.max_weight_matching(h, maxcardinality=True)) == h.number_of_nodes():
                out.add((min(a, b), max(a, b)))
    return out


@pytest.mark.parametrize("name", ["drd2", "generated", "big"])
def test_every_bond_of_g_prime_against_networkx(golden_dir, name):
    inp, rules, res, traces = model_of(name, golden_dir)
    n_bonds = n_deloc = with_deloc = 0
    unread = 0
    for g, trace in enumerate(traces):
        if name == "generated" and res["status"][g] == XM.RES_EMPTY:        # a string the reader found no structure for
            unread += 1
            continue
        assert res["status"][g] == 0 and trace, g
        got = {(a, b) for (a, b) in trace["bonds"] if a < b}
        assert got == nx_verdicts(trace), (name, g)
        assert got == bonds_in(res["delocalized"][g], inp["nodes"].shape[1])
        n_bonds += len(trace["order"]) // 2
        n_deloc += len(got)
        with_deloc += bool(got)
        assert res["n_systems"][g] == nx.number_connected_components(nx.Graph(list(got))), (name, g)
        for a, b in got:                                                    # only ring bonds
            h = nx.Graph((x, y) for (x, y) in trace["order"] if x < y)
            h.remove_edge(a, b)
            assert nx.has_path(h, a, b), (name, g, a, b)
    if name == "drd2":
        assert len(traces) == 863 and with_deloc == 853                     # the issue's count
    if name == "generated":
        assert len(traces) == 512 and unread == 309                         # the 309 without a Kekule structure
    if name == "big":
        assert res["n_delocalized"][0] == 128 and len(traces[1]["order"]) // 2 == 159 > 128
        assert res["n_delocalized"][1] > 128 and traces[1]["counters"]["searches"] < 159


def test_phase_invariance_on_the_drd2_molecules(golden_dir):
    inp, rules, res, traces = model_of("drd2", golden_dir)
    edges2, changed = rephased_drd2(golden_dir)
    res2 = XM.resonance(inp["nodes"], edges2, inp["n_nodes"], rules)
    for name in res:
        assert np.array_equal(res[name], res2[name]), name                  # byte for byte, all 863
    assert len(changed) == PHASES_CHANGED
    pairs = changed[:200]
    stored_a = CM.canonical(inp["nodes"][pairs], inp["edges"][pairs], inp["n_nodes"][pairs])
    stored_b = CM.canonical(inp["nodes"][pairs], edges2[pairs], inp["n_nodes"][pairs])
    same_stored = sum(np.array_equal(stored_a["edges"][k], stored_b["edges"][k]) and
                      np.array_equal(stored_a["nodes"][k], stored_b["nodes"][k]) for k in range(len(pairs)))
    normal = CM.canonical(inp["nodes"][pairs], res["edges"][pairs], inp["n_nodes"][pairs])
    normal2 = CM.canonical(inp["nodes"][pairs], res2["edges"][pairs], inp["n_nodes"][pairs])
    assert np.array_equal(normal["key"], normal2["key"]) and np.array_equal(normal["edges"], normal2["edges"])
    assert same_stored == PAIRS_EQUAL_AS_STORED < 200
    # valence-neutral: the bond-order sums of the stored molecule, of the other phase and of the normal form's inverse
    o2 = np.array(rules.order2)
    assert np.array_equal((inp["edges"] * o2).sum(axis=(2, 3)), (edges2 * o2).sum(axis=(2, 3)))


#: what the model gave when this test was written (seed 20261021); the issue's prototype, with draws of its own, found
#: 589 re-phased molecules and 42 of the first 200 pairs equal as stored
PHASES_CHANGED = 609
PAIRS_EQUAL_AS_STORED = 38


def test_the_converse_on_hand_cases():
    """Equal normal forms mean perfect matchings of one G': two molecules that differ OUTSIDE G' differ in normal form,
    and so do two whose double bonds are not a matching of the same G' (the quinoid and the benzenoid ring)."""
    rules = hand_rules()
    benzenoid = hand_molecule("CCCCCCCC", ring_bonds(6) + [(0, 6, 1), (3, 7, 1)], rules)
    quinoid = hand_molecule("CCCCCCCC", [(0, 6, 2), (3, 7, 2), (0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 2),
                                         (5, 0, 1)], rules)
    a, b = XM.resonance_one(*benzenoid, 8, rules), XM.resonance_one(*quinoid, 8, rules)
    assert not np.array_equal(a["edges"], b["edges"]) and a["n_delocalized"] == 6 and b["n_delocalized"] == 0
    inp, _, res, traces = model_of("hand")
    names = list(HAND)
    for x in range(len(names)):
        for y in range(x + 1, len(names)):
            if np.array_equal(res["edges"][x], res["edges"][y]) and np.array_equal(inp["nodes"][x], inp["nodes"][y]):
                assert traces[x]["adj"] == traces[y]["adj"] and traces[x]["in_v"] == traces[y]["in_v"], (names[x], names[y])
                assert {names[x], names[y]} == {"naphthalene_central", "naphthalene_outer"}


def test_round_trips(golden_dir):
    inp, rules, res, traces = model_of("drd2", golden_dir)
    pick = list(range(0, 863, 9))
    nodes, edges, n = inp["nodes"][pick], inp["edges"][pick], inp["n_nodes"][pick]
    k = XM.kekulize(nodes, res["edges"][pick], n, rules)
    assert not k["status"].any()
    again = XM.resonance(nodes, k["edges"], n, rules)
    for name in again:
        assert np.array_equal(again[name], res[name][pick]), name           # resonance(kekulize(resonance(m))) == resonance(m)
    o2 = np.array(rules.order2)
    assert np.array_equal((k["edges"] * o2).sum(axis=(2, 3)), (edges * o2).sum(axis=(2, 3)))   # every atom's order sum
    v0, v1 = VM.validity(nodes, edges, n, rules), VM.validity(nodes, k["edges"], n, rules)
    for name in v0:
        assert np.array_equal(v0[name], v1[name]), name                     # and the validity model's whole verdict


def test_canonical_compound_under_node_orders_and_phases(golden_dir):
    inp, rules, res, traces = model_of("drd2", golden_dir)
    edges2, changed = rephased_drd2(golden_dir)
    rng = np.random.default_rng(7)
    for g in changed[:6]:
        n = int(inp["n_nodes"][g])
        forms = []
        for phase in (inp["edges"][g], edges2[g]):
            for _ in range(8):
                perm = rng.permutation(n)
                pn, pe = CM.permute(inp["nodes"][g], phase, perm)
                forms.append(XM.canonical_compound(pn[None], pe[None], np.array([n]), rules))
        for f in forms[1:]:
            for name in ("nodes", "edges", "key", "status"):
                assert np.array_equal(f[name], forms[0][name]), (g, name)
        assert forms[0]["status"][0] == 0
        # the canonical Kekule structure is a Kekule structure of the same compound: its normal form is the canonical one
        back = XM.resonance(forms[0]["nodes"], forms[0]["edges"], np.array([n]), rules)
        can = CM.canonical(inp["nodes"][g][None], res["edges"][g][None], np.array([n]))
        assert np.array_equal(back["edges"], can["edges"]), g
        _CACHE.setdefault("compound_forms", {})[g] = forms[0]


def test_smiles_of_the_canonical_compound_are_equal_and_read_back(golden_dir):
    """The writer's strings of ``canonical_compound``'s forms: one string per compound whatever the node order and the
    stored phase, and the reader's molecule of that string is the same compound."""
    from tests import smiles_read_model as RM
    inp, rules, res, traces = model_of("drd2", golden_dir)
    edges2, changed = rephased_drd2(golden_dir)
    rng = np.random.default_rng(11)
    for g in changed[:4]:
        n = int(inp["n_nodes"][g])
        strings = set()
        for phase in (inp["edges"][g], edges2[g]):
            for _ in range(2):
                perm = rng.permutation(n)
                pn, pe = CM.permute(inp["nodes"][g], phase, perm)
                form = XM.canonical_compound(pn[None], pe[None], np.array([n]), rules)
                out = SM.write_batch(form["nodes"], form["edges"], np.array([n]), rules)
                assert out["status"][0] == 0
                strings.add(out["strings"][0])
        assert len(strings) == 1, (g, strings)
        text, length = RM.pack([strings.pop()])
        back = RM.read_one(text[0], int(length[0]), rules, DRD2_N, sum(rules.groups), len(rules.order2))
        assert back["status"] & RM.RD_ERROR == 0 and back["n_nodes"] == n
        a = XM.canonical_compound(back["nodes"][None], back["edges"][None], np.array([n]), rules)
        b = XM.canonical_compound(inp["nodes"][g][None], inp["edges"][g][None], np.array([n]), rules)
        assert np.array_equal(a["key"], b["key"]) and np.array_equal(a["edges"], b["edges"]), g


HARNESS = r"""
#include <cstdio>
#include <vector>
#include "gi_res_search.h"
struct Marks {
    unsigned (*row)[4];
    void mark(int a, int b) { row[a][b >> 5] |= 1u << (b & 31); row[b][a >> 5] |= 1u << (a & 31); }
    bool marked(int a, int b) const { return (row[a][b >> 5] >> (b & 31)) & 1u; }
};
int main() {
    char mode;
    while (std::scanf(" %c", &mode) == 1) {
        int n;
        if (std::scanf("%d", &n) != 1 || n < 0 || n > 128) return 2;
        if (mode == 'R') {                                   // mate [n], rows [n][4] -> del [n][4], searches
            const int st = 3;                                // an interleaved workspace, as the lanes of a workgroup have
            std::vector<unsigned char> mate(n + 1), parent(n * st + 1), base(n * st + 1), queue(n * st + 1);
            std::vector<unsigned> rows(n * 4 + 4);
            static unsigned del[128][4];
            for (int i = 0; i < n; ++i) { int m; if (std::scanf("%d", &m) != 1) return 2; mate[i] = (unsigned char)m; }
            for (int i = 0; i < n * 4; ++i) if (std::scanf("%u", &rows[i]) != 1) return 2;
            for (int i = 0; i < 128; ++i) for (int w = 0; w < 4; ++w) del[i][w] = 0u;
            Marks d = {del};
            int searches = 0;
            for (int a = 0; a < n; ++a) searches += res_doubles(rows.data(), n, mate.data(), a, parent.data(), base.data(), queue.data(), st, d);
            for (int u = 0; u < n; ++u) searches += res_singles(rows.data(), n, mate.data(), u, parent.data(), base.data(), queue.data(), st, d);
            for (int i = 0; i < n; ++i) for (int w = 0; w < 4; ++w) std::printf("%u ", del[i][w]);
            std::printf("%d\n", searches);
        } else {                                             // 'K': rows [n][4] -> ok, mate [n], counters [3]
            std::vector<unsigned char> mate(n + 1), parent(n + 1), base(n + 1), queue(n + 1);
            std::vector<unsigned> rows(n * 4 + 4);
            for (int i = 0; i < n * 4; ++i) if (std::scanf("%u", &rows[i]) != 1) return 2;
            int counters[3] = {0, 0, 0};
            const bool ok = res_match(rows.data(), n, mate.data(), parent.data(), base.data(), queue.data(), counters);
            std::printf("%d ", ok ? 1 : 0);
            for (int i = 0; i < n; ++i) std::printf("%d ", (int)mate[i]);
            std::printf("%d %d %d\n", counters[0], counters[1], counters[2]);
        }
    }
    return 0;
}
"""


def rows_of(n, adj):
    rows = np.zeros((n, 4), np.uint32)
    for i in range(n):
        for j in adj[i]:
            rows[i, j >> 5] |= np.uint32(1 << (j & 31))
    return rows


def test_the_host_device_search_on_the_host(golden_dir, tmp_path):
    """csrc/gi_res_search.h compiled for the host (under ASan and UBSan where the compiler has them) against the model:
    the delocalised rows of every molecule of the inputs above — every bond of every G' — and `match` on the
    channel-Fe graphs of their normal forms and on the reader's candidate graphs of the generated ring systems."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    cfile, exe = tmp_path / "res_search.cpp", tmp_path / "res_search"
    cfile.write_text(HARNESS)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", CSRC, str(cfile), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (no sanitizer runtime to link against: plain build)
        subprocess.run(base, check=True)
    lines, expect = [], []
    from tests import kekule_read_model as KM
    n_bonds = 0
    for name in ("hand", "drd2", "generated", "big"):
        inp, rules, res, traces = model_of(name, golden_dir)
        for g, trace in enumerate(traces):
            if not trace:
                continue
            n = trace["n"]
            mate = [255 if m < 0 else m for m in trace["mate"]]
            lines.append("R %d %s %s" % (n, " ".join(map(str, mate)), " ".join(map(str, rows_of(n, trace["adj"]).reshape(-1)))))
            expect.append(("R", res["delocalized"][g].view(np.uint32)[:n].reshape(-1).tolist(), trace["counters"]["searches"]))
            n_bonds += len(trace["order"]) // 2
            marked = [[b for (a, b) in sorted(trace["bonds"]) if a == i] for i in range(n)]
            counters = {}
            m = KM.match(n, [bool(x) for x in marked], marked, counters)
            lines.append("K %d %s" % (n, " ".join(map(str, rows_of(n, marked).reshape(-1)))))
            expect.append(("K", m, counters))
    for trace in generated_model()[1]:                          # the reader's graphs: odd cycles, blossoms, failures
        if "cand" not in trace or trace["need"] != [bool(c) for c in trace["cand"]]:
            continue                                                        # (res_match: an atom needs iff it has a candidate)
        n = trace["n"]
        lines.append("K %d %s" % (n, " ".join(map(str, rows_of(n, trace["cand"]).reshape(-1)))))
        expect.append(("K", trace["mate"], trace["counters"]))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert len(got) == len(expect) and n_bonds > 15000
    blossoms = failures = 0
    for k, (line, want) in enumerate(zip(got, expect)):
        v = [int(x) for x in line.split()]
        if want[0] == "R":
            assert v[:-1] == want[1], k
            assert v[-1] == want[2], k                                      # the same searches as the model makes
        else:
            mate, counters = want[1], want[2]
            blossoms += counters["blossoms"]
            if mate is None:
                failures += 1
                assert v[0] == 0, k
            else:
                assert v[0] == 1 and v[1:-3] == [255 if m < 0 else m for m in mate], k
                assert v[-3:] == [counters["greedy"], counters["searches"], counters["augmentations"]], k
    assert blossoms > 0 and failures > 0


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    for name, n_args in (("gi_mol_resonance", 20), ("gi_mol_kekulize", 16)):
        decl = re.search(rf"^int\s+{name}\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
        assert name in L.SIGNATURES and hasattr(lib, name)
        assert len(L.SIGNATURES[name][1]) == len(decl.split(",")) == n_args
    for name, value in (("EMPTY", "128"), ("SELF_LOOP", "256"), ("AROMATIC", "2048"), ("BOND_ORDER", r"\(1 << 22\)"),
                        ("NO_KEKULE", r"\(1 << 26\)")):
        assert re.search(rf"#define\s+GI_RES_{name}\s+{value}", hdr), name
    assert (L.RES_EMPTY, L.RES_SELF_LOOP, L.RES_AROMATIC, L.RES_BOND_ORDER, L.RES_NO_KEKULE) == \
        (XM.RES_EMPTY, XM.RES_SELF_LOOP, XM.RES_AROMATIC, XM.RES_BOND_ORDER, XM.RES_NO_KEKULE)
    assert XM.UNSOUND == analyze.MALFORMED_BITS | L.RES_EMPTY | L.RES_SELF_LOOP
    assert XM.KEKULE_ERROR == analyze.NO_KEKULE_BITS
    assert set(analyze.RESONANCE_STATUS_MESSAGES) == {1, 2, 8, 16, 32, 64, 128, 256, 2048, 1 << 22, 1 << 26}
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # added entry points are compatible
    src = open(os.path.join(CSRC, "gi_resonance.hip")).read()
    assert "gi_resonance.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert "getenv" not in src and "gi_read_labelled<false>" in src and "gi_res_search.h" in src
    assert "gi_mol_resonance" in open(os.path.join(ROOT, "INTEGRATION.md")).read()

    def res(G=0, N=72, Fn=14, Fe=3, dtype=1, nb=1, A=7, C=3, H=4, edges_out=None):
        return lib.gi_mol_resonance(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, None, None, None, None,
                                    None, edges_out, None)

    def kek(G=0, N=72, Fn=14, Fe=3, dtype=1, nb=1, A=7, C=3, H=4):
        return lib.gi_mol_kekulize(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, None, None, None)
    for call in (res, kek):                                                # nothing is launched for any of these
        assert call() == 0 and call(G=1) == -1 and call(G=-1) == -1 and call(N=129) == -1 and call(N=0) == -1
        assert call(Fn=513) == -2 and call(dtype=2) == -1 and call(nb=2) == -1 and call(A=8) == -1 and call(A=0) == -1
    assert res(Fe=9) == -1 and res(Fe=8) == 0 and res(Fe=8, edges_out=1) == -2 and res(Fe=7, edges_out=1) == 0
    assert kek(Fe=8) == -2 and kek(Fe=7) == 0 and kek(Fe=0) == -1


def test_python_boundary_raises():
    n, e = torch.zeros(2, 72, 14, dtype=torch.int8), torch.zeros(2, 72, 72, 3, dtype=torch.int8)
    host_rules = analyze.ValenceRules(device=None, **DRD2_ARGS)
    for fn in (analyze.resonance, analyze.kekulize, analyze.canonical_compound):
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(n, e, None, host_rules)
        with pytest.raises(TypeError, match="tensor"):
            fn(n.numpy(), e.numpy(), None, host_rules)
        with pytest.raises(TypeError, match="ValenceRules"):
            fn(n, e, None, [7, 3, 4])
    wide = torch.zeros(2, 72, 72, 8, dtype=torch.int8)
    rules8 = analyze.ValenceRules(device=None, bond_orders=(1, 2, 3, 1.5, 1, 1, 1, 1), **DRD2_ARGS)
    with pytest.raises(ValueError, match="one channel more"):              # Fe = 8: before anything is launched
        analyze.resonance(n, wide, None, rules8)
    with pytest.raises(ValueError, match="one channel more"):
        analyze.canonical_compound(n, wide, None, rules8)
    with pytest.raises(RuntimeError, match="no CPU"):                      # without the edges Fe = 8 is within the limits
        analyze.resonance(n, wide, None, rules8, want_edges=False)
    with pytest.raises(ValueError, match="one channel more"):
        analyze.kekulize(n, torch.zeros(2, 72, 72, 9, dtype=torch.int8), None, rules8)
    assert analyze.ResonanceForms.nbytes(0, 72) == 0 and analyze.ResonanceForms.nbytes(3, 13) == 4 * (4 * 3 + 3 * 13 * 4)
    assert analyze.describe_resonance_status(0) == "well-formed" and "Kekule" in analyze.describe_resonance_status(1 << 26)
    if not torch.cuda.is_available():
        return
    dn, de = n.cuda(), e.cuda()                                            # raised before anything is launched
    rules = analyze.ValenceRules(**DRD2_ARGS)
    for fn in (analyze.resonance, analyze.kekulize):
        with pytest.raises(RuntimeError, match="device=None"):
            fn(dn, de, None, host_rules)
        with pytest.raises(ValueError, match="contiguous"):
            fn(dn, de.transpose(1, 2), None, rules)
        with pytest.raises(TypeError, match="float32 or both int8"):
            fn(dn.float(), de, None, rules)
        with pytest.raises(ValueError, match="does not match"):
            fn(dn, de[:, :71], None, rules)
        with pytest.raises(RuntimeError, match="n_nodes"):
            fn(dn, de, torch.zeros(2, dtype=torch.int32), rules)
    with pytest.raises(ValueError, match="bond"):                          # the rules hold three orders, the input two
        analyze.kekulize(dn, de, None, rules)
    with pytest.raises(ValueError, match="one channel more"):
        analyze.resonance(dn, wide.cuda(), None, analyze.ValenceRules(bond_orders=(1, 2, 3, 1.5, 1, 1, 1, 1), **DRD2_ARGS))
