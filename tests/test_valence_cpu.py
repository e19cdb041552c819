"""CPU: molecule validity's numpy model, rules table, golden, binding and Python boundary
(graphinvent_amd.analyze.ValenceRules / validity / fraction_valid).  No device compute is issued.

The numpy model (tests/valence_model.py) is the specification the device is held to exactly.  It is a valence test of the
labelled graph with a table of our own; no parity with RDKit is claimed (there is no RDKit to compare with).  Here it is
pinned to textbook cases built inline and to what the SMILES strings of the reference's 30 shipped molecules say
(tests/golden/golden_valence.npz, tests/golden/make_golden_valence.py)."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import valence_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the segment tables of the stored sets (golden_routes.npz) and of the generated ones (golden_grow.npz)
RULE_ARGS = {
    "gdb13": dict(atom_types=["C", "N", "O", "S", "Cl"], formal_charge=[-1, 0, 1]),
    "arom5": dict(atom_types=["C", "N", "O", "S"], formal_charge=[-1, 0, 1], imp_H=[0, 1, 2, 3],
                  bond_orders=(1, 2, 3, 1.5)),
    "chiral6": dict(atom_types=["C", "N", "O"], formal_charge=[0, 1], imp_H=[0, 1, 2], bond_orders=(1, 2, 3, 1.5)),
    "atoms_charges": dict(atom_types=["C", "N", "O", "S"], formal_charge=[-1, 0, 1]),
    "imp_h_chirality": dict(atom_types=["C", "N", "O"], formal_charge=[0, 1], imp_H=[0, 1, 2], bond_orders=(1, 2)),
    "chem": dict(atom_types=["C", "N", "O", "S", "Cl", "F", "H"], formal_charge=[-1, 0, 1]),
}
_CACHE = {}


def model_rules(name):
    """The model's rules of a set, checked once against the tables the library builds from the same arguments."""
    if ("rules", name) not in _CACHE:
        model, lib_rules = VM.Rules(**RULE_ARGS[name]), analyze.ValenceRules(device=None, **RULE_ARGS[name])
        assert lib_rules.mask_table.tolist() == [[sum(1 << v for v in vals) for vals in row] for row in model.allowed]
        assert lib_rules.mass_table.tolist() == model.mass and lib_rules.mass_h == model.mass_h
        assert lib_rules.groups == model.groups and lib_rules.h_type == model.h_type
        assert lib_rules.imp_H == model.h_values
        assert lib_rules.order2_tables[len(model.order2)].tolist() == model.order2
        _CACHE[("rules", name)] = model
    return _CACHE[("rules", name)]


def stored_set(golden_dir, c):
    """(nodes, edges, n_nodes or None, termination or None) of a stored set."""
    if c in ("gdb13", "arom5", "chiral6"):
        if "routes" not in _CACHE:
            _CACHE["routes"] = np.load(os.path.join(golden_dir, "golden_routes.npz"))
        R = _CACHE["routes"]
        return R[f"{c}::mol_nodes"], R[f"{c}::mol_edges"], None, None
    if "grow" not in _CACHE:
        _CACHE["grow"] = np.load(os.path.join(golden_dir, "golden_grow.npz"))
    R = _CACHE["grow"]
    return (R[f"{c}::generated_nodes"], R[f"{c}::generated_edges"], R[f"{c}::generated_n_nodes"],
            R[f"{c}::properly_terminated"])


def model_of(golden_dir, c):
    """The model's result on set c, computed once and shared (read only)."""
    if ("model", c) not in _CACHE:
        nodes, edges, n, term = stored_set(golden_dir, c)
        _CACHE[("model", c)] = VM.validity(nodes, edges, n, model_rules(c), termination=term)
    return _CACHE[("model", c)]


def shipped(golden_dir):
    """The 30 whole molecules of the shipped debug set, in golden_valence.npz's order, and that file."""
    if "shipped" not in _CACHE:
        V = np.load(os.path.join(golden_dir, "golden_valence.npz"))
        nodes, edges = [], []
        for split in V["splits"]:
            d = np.load(os.path.join(golden_dir, f"gdb13_1K-debug_{split}.npz"))
            whole = np.flatnonzero(d["APDs"][:, -1] > 0)
            nodes.append(d["nodes"][whole].astype(np.int8))
            edges.append(d["edges"][whole].astype(np.int8))
        _CACHE["shipped"] = (np.concatenate(nodes), np.concatenate(edges), V)
    return _CACHE["shipped"]


def chemistry_table():
    """name -> (nodes, edges, valid?, {atom: fill}) on N = 8, the "chem" rules: textbook cases."""
    r = model_rules("chem")
    star = lambda centre, leaf, k, order=1: ([centre] + [leaf] * k, [(0, i + 1, order) for i in range(k)])
    cases = {
        "methane": ([("C", 0)], [], True, {0: 4}),
        "ammonium_like": (*star(("N", 1), ("C", 0), 4), True, {0: 0, 1: 3}),
        "nitro": ([("C", 0), ("N", 1), ("O", 0), ("O", -1)], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], True,
                  {0: 3, 1: 0, 2: 0, 3: 0}),
        "oxonium": (*star(("O", 1), ("C", 0), 3), True, {0: 0}),
        "alkoxide": ([("C", 0), ("O", -1)], [(0, 1, 1)], True, {0: 3, 1: 0}),
        "sf6": (*star(("S", 0), ("F", 0), 6), True, {0: 0, 1: 0}),
        "chloride": ([("Cl", -1)], [], True, {0: 0}),
        "hydrogen_cyanide": ([("H", 0), ("C", 0), ("N", 0)], [(0, 1, 1), (1, 2, 3)], True, {0: 0, 1: 0, 2: 0}),
        "sulfoxide_like": ([("C", 0), ("S", 0), ("O", 0)], [(0, 1, 1), (1, 2, 2)], True, {1: 1}),   # S: 3 -> 4
        "five_bonded_c": (*star(("C", 0), ("F", 0), 5), False, {}),
        "five_valent_n": ([("N", 0), ("O", 0), ("O", 0), ("C", 0)], [(0, 1, 2), (0, 2, 2), (0, 3, 1)], False, {}),
        "two_bonded_cl": ([("C", 0), ("Cl", 0), ("C", 0)], [(0, 1, 1), (1, 2, 1)], False, {}),
        "empty": ([], [], False, {}),
    }
    out = {}
    for name, (atoms, bonds, ok, fills) in cases.items():
        out[name] = (*VM.molecule(8, r, atoms, bonds), ok, fills)
    nodes, edges = VM.molecule(8, r, [("C", 0), ("C", 0)], [(0, 1, 1)])
    edges[1, 1, 0] = 1
    out["self_loop"] = (nodes, edges, False, {})
    return out


def status_cases():
    """name -> (nodes, edges, n_nodes, expected status) on N = 6, the "gdb13" rules: one hand-made molecule per bit."""
    r = model_rules("gdb13")
    base = lambda: VM.molecule(6, r, [("C", 0), ("N", 0), ("O", 0)], [(0, 1, 1), (1, 2, 1)])
    cases = {"sound": (*base(), 3, 0)}
    nodes, edges = base(); nodes[1, 2] = 1                                # N and O at once
    cases["onehot_two"] = (nodes, edges, 3, L.MOL_ONEHOT)
    nodes, edges = base(); nodes[2, 5:8] = 0                              # no charge entry
    cases["onehot_none"] = (nodes, edges, 3, L.MOL_ONEHOT)
    nodes, edges = base(); edges[1, 4, 0] = edges[4, 1, 0] = 1
    cases["bond_past_n"] = (nodes, edges, 3, L.MOL_BOND_PAST_N)
    nodes, edges = base(); edges[0, 1, 0] = edges[1, 0, 0] = 3
    cases["value"] = (nodes, edges, 3, L.MOL_VALUE)
    nodes, edges = base(); edges[0, 1, 1] = edges[1, 0, 1] = 1
    cases["multi_bond"] = (nodes, edges, 3, L.MOL_MULTI_BOND)
    nodes, edges = base(); edges[0, 2, 0] = 1
    cases["asymmetric"] = (nodes, edges, 3, L.MOL_ASYMMETRIC)
    nodes, edges = base(); nodes[4, 0] = nodes[4, 6] = 1
    cases["node_past_n"] = (nodes, edges, 3, L.MOL_NODE_PAST_N)
    cases["n_too_large"] = (*base(), 7, L.MOL_NODE_PAST_N | L.MOL_ONEHOT)        # rows 3 .. 5 are empty
    nodes, edges = base()
    cases["empty"] = (nodes * 0, edges * 0, 0, L.VAL_EMPTY)
    nodes, edges = base(); edges[0, 0, 0] = 1
    cases["self_loop"] = (nodes, edges, 3, L.VAL_SELF_LOOP)
    cases["over"] = (*VM.molecule(6, r, [("O", 0), ("C", 0), ("C", 0)], [(0, 1, 2), (0, 2, 1)]), 3, L.VAL_OVER)
    cases["fragments"] = (*VM.molecule(6, r, [("C", 0), ("C", 0), ("O", 0)], [(0, 1, 1)]), 3, L.VAL_FRAGMENTS)
    return cases


def aromatic_and_h_cases():
    """(nodes, edges, expected status, expected fills) on the "arom5" rules (an implicit-H segment, order 1.5)."""
    r = model_rules("arom5")
    ring = [(i, (i + 1) % 6, 1.5) for i in range(6)]
    nodes, edges = zip(VM.molecule(13, r, [("C", 0, 1)] * 6, ring),                     # benzene: 3 per 2, fill 1
                       VM.molecule(13, r, [("C", 0, 0)] * 6, ring),                     # ... stored as 0 H
                       VM.molecule(13, r, [("C", 0, 3), ("O", 0, 1)], [(0, 1, 1)]),     # methanol, stored right
                       VM.molecule(13, r, [("C", 0, 3), ("O", 0, 0)], [(0, 1, 1)]))     # O stored without its H
    return (np.stack(nodes), np.stack(edges),
            [L.VAL_AROMATIC, L.VAL_AROMATIC | L.VAL_H_MISMATCH, 0, L.VAL_H_MISMATCH], [1, 1, 3, 3])


# ---- the model ------------------------------------------------------------------------------------------------

def test_model_on_textbook_cases():
    r = model_rules("chem")
    for name, (nodes, edges, ok, fills) in chemistry_table().items():
        res = VM.judge(nodes, edges, None, r)
        assert bool(res["valid"]) == ok, (name, res)
        for atom, h in fills.items():
            assert res["atom_h"][atom] == h, (name, atom, res["atom_h"])
    t = chemistry_table()
    methane = VM.judge(*t["methane"][:2], None, r)
    assert methane["desc"].tolist() == [1, 4, 12011 + 4 * 1008, 0, 1, 0] and methane["atom_valence"][0] == 0
    hcn = VM.judge(*t["hydrogen_cyanide"][:2], None, r)                  # an explicit H counts in n_h, with its own mass
    assert hcn["desc"].tolist() == [3, 1, 1008 + 12011 + 14007, 2, 1, 0]
    assert VM.judge(*t["five_bonded_c"][:2], None, r)["status"] == VM.VAL_OVER
    assert VM.judge(*t["five_bonded_c"][:2], None, r)["first_bad"] == 0
    assert VM.judge(*t["two_bonded_cl"][:2], None, r)["first_bad"] == 1
    assert VM.judge(*t["five_valent_n"][:2], None, r)["atom_valence"][0] == 5
    assert VM.judge(*t["empty"][:2], None, r)["status"] == VM.VAL_EMPTY
    loop = VM.judge(*t["self_loop"][:2], None, r)
    assert loop["status"] == VM.VAL_SELF_LOOP and loop["valid"] == 0 and loop["atom_valence"][1] == 2


def test_model_status_bits_and_fragments():
    r = model_rules("gdb13")
    for name, (nodes, edges, n, want) in status_cases().items():
        for given in (n, None) if name not in ("n_too_large", "onehot_none") else (n,):
            res = VM.judge(nodes, edges, given, r)
            assert res["status"] == want, (name, given, res["status"])
            assert bool(res["valid"]) == (name in ("sound", "fragments")), name
            if want & VM.MALFORMED:
                assert (res["atom_valence"] == -1).all() and (res["atom_h"] == -1).all() and not res["desc"].any()
    nodes, edges, n, _ = status_cases()["fragments"]
    loose, strict = VM.judge(nodes, edges, n, r), VM.judge(nodes, edges, n, r, require_connected=True)
    assert loose["valid"] == 1 and strict["valid"] == 0 and loose["status"] == strict["status"] == VM.VAL_FRAGMENTS
    assert loose["desc"].tolist() == [3, 3 + 3 + 2, 2 * 12011 + 15999 + 8 * 1008, 1, 2, 0]
    nodes, edges, want, fills = aromatic_and_h_cases()
    res = VM.validity(nodes, edges, None, model_rules("arom5"))
    assert res["status"].tolist() == want and res["atom_h"][:, 0].tolist() == fills and res["valid"].all()
    assert res["atom_valence"][0, :6].tolist() == [3] * 6 and res["desc"][0].tolist() == [6, 6, 78114, 6, 1, 1]


def test_model_on_the_shipped_molecules(golden_dir):
    nodes, edges, V = shipped(golden_dir)
    assert len(nodes) == 30 and list(V["elements_order"]) == RULE_ARGS["gdb13"]["atom_types"]
    res = VM.validity(nodes, edges, None, model_rules("gdb13"))
    assert res["valid"].tolist() == [1.0] * 30 and not res["status"].any()           # all valid, none fragmented
    assert (res["desc"][:, 4] == 1).all() and res["counts"].tolist() == [30, 0, 0, 30]
    want = {k: np.concatenate([V[f"{s}::{k}"] for s in V["splits"]]) for k in ("elements", "ring_pairs", "n_h")}
    assert np.array_equal(nodes[:, :, :5].sum(axis=1), want["elements"])
    assert np.array_equal(res["desc"][:, 0], want["elements"].sum(axis=1))
    assert np.array_equal(res["desc"][:, 1], want["n_h"]) and np.array_equal(res["desc"][:, 5], want["ring_pairs"])
    assert not nodes[:, :, 5].any() and not nodes[:, :, 7].any()                     # no charged atom
    assert V["train::smiles"][0] == "CC1C2N1CC1=C2CC=C1"                             # C9H11N, three rings
    assert res["desc"][0].tolist() == [10, 11, 9 * 12011 + 14007 + 11 * 1008, 12, 1, 3]


def test_model_on_the_stored_sets_has_something_to_find(golden_dir):
    res = model_of(golden_dir, "gdb13")
    assert res["valid"][:20].all() and 0 < res["valid"].sum() < 140 and (res["status"] & VM.VAL_OVER != 0).sum() > 50
    assert not (res["status"] & VM.MALFORMED).any()
    assert (model_of(golden_dir, "arom5")["status"] & VM.VAL_AROMATIC).any()
    assert (model_of(golden_dir, "arom5")["status"] & VM.VAL_H_MISMATCH).any()
    assert (model_of(golden_dir, "chiral6")["desc"][:, 0] > 32).any()
    for c in ("atoms_charges", "imp_h_chirality"):
        res = model_of(golden_dir, c)
        assert 0 < res["counts"][1] < res["counts"][3] and res["counts"][2] <= min(res["counts"][:2]), (c, res["counts"])


def test_fraction_valid_restatement():
    valid, term = np.array([1, 0, 1, 1, 0], np.float32), np.array([1, 1, 0, 1, 0], np.int8)
    assert VM.fraction_valid(valid, term) == (np.float32(3) / np.float32(5), np.float32(2) / np.float32(3),
                                              np.float32(3) / np.float32(5))
    assert VM.fraction_valid(valid, term * 0) == (np.float32(0.6), np.float32(0.0), np.float32(0.0))
    # the library's quotients from the same counts (its arithmetic is plain torch on the counts, wherever they live)
    for t in (term, term * 0):
        res = analyze.MoleculeValidity(torch.zeros(analyze.MoleculeValidity.nbytes(5, 3), dtype=torch.uint8), 5, 3)
        res.counts.copy_(torch.tensor([3, int(t.sum()), int(((valid != 0) & (t != 0)).sum()), 5], dtype=torch.int32))
        got = analyze.fraction_valid(res)
        assert all(f.dtype == torch.float32 and f.dim() == 0 for f in got)
        assert tuple(np.float32(f.item()) for f in got) == VM.fraction_valid(valid, t)
    empty = analyze.MoleculeValidity(torch.zeros(16, dtype=torch.uint8), 0, 3)
    assert [float(f) for f in analyze.fraction_valid(empty)] == [0.0, 0.0, 0.0]


# ---- the rules ------------------------------------------------------------------------------------------------

def test_default_rules_entry_by_entry():
    neutral = {"H": (1,), "B": (3,), "C": (4,), "Si": (4,), "N": (3,), "P": (3, 5), "O": (2,), "S": (2, 4, 6),
               "Se": (2, 4, 6), "F": (1,), "Cl": (1,), "Br": (1,), "I": (1,)}
    charged = {("N", 1): (4,), ("O", 1): (3,), ("N", -1): (2,), ("O", -1): (1,), ("C", -1): (3,), ("C", 1): (3,),
               ("B", -1): (4,), ("S", 1): (3, 5), ("Cl", -1): (0,), ("Cl", 1): (2, 4, 6), ("H", 1): (0,), ("H", -1): (0,),
               ("P", 1): (4,), ("P", -1): (2, 4, 6), ("Si", -1): (3, 5), ("F", -1): (0,), ("Br", 1): (2, 4, 6),
               ("Se", -1): (1,), ("I", -1): (0,)}
    masses = {"H": 1008, "B": 10810, "C": 12011, "N": 14007, "O": 15999, "F": 18998, "Si": 28085, "P": 30974,
              "S": 32060, "Cl": 35450, "Se": 78971, "Br": 79904, "I": 126904}
    assert analyze.DEFAULT_MASSES == masses == VM.MASSES
    for sym, vals in neutral.items():
        assert analyze.default_valences(sym, 0) == vals == VM.valences_of(sym, 0), sym
    for (sym, c), vals in charged.items():
        assert analyze.default_valences(sym, c) == vals == VM.valences_of(sym, c), (sym, c)
    for sym in masses:                                                   # the two statements agree everywhere
        for c in (-2, -1, 0, 1, 2):
            assert analyze.default_valences(sym, c) == VM.valences_of(sym, c), (sym, c)
    assert analyze.default_valences("B", 1) is None and analyze.default_valences("C", 2) is None
    assert analyze.default_valences("Fe", 0) is None
    rules = analyze.ValenceRules(list(neutral), [-1, 0, 1], allowed={("B", 1): (2,)}, device=None)
    for a, sym in enumerate(neutral):
        for c, charge in enumerate([-1, 0, 1]):
            vals = {("B", 1): (2,)}.get((sym, charge)) or VM.valences_of(sym, charge)
            assert rules.valences[(sym, charge)] == vals
            assert int(rules.mask_table[a, c]) == sum(1 << v for v in vals), (sym, charge)
        assert int(rules.mass_table[a]) == masses[sym]
    assert rules.groups == (13, 3, 0) and rules.h_type == 0 and rules.mass_h == 1008
    assert {k: v.tolist() for k, v in rules.order2_tables.items()} == {3: [2, 4, 6], 4: [2, 4, 6, 3]}
    assert rules.mask_table.dtype == np.uint16 and rules.mass_table.dtype == np.int32
    for name, kw in RULE_ARGS.items():                                   # the tests' rules: library == model
        lib_rules, model = analyze.ValenceRules(device=None, **kw), model_rules(name)
        assert [[int(m) for m in row] for row in lib_rules.mask_table] == \
            [[sum(1 << v for v in vals) for vals in row] for row in model.allowed], name
        assert lib_rules.mass_table.tolist() == model.mass and lib_rules.groups == model.groups
        assert lib_rules.h_type == model.h_type and lib_rules.imp_H == model.h_values
        if "bond_orders" in kw:
            assert lib_rules.order2_tables[len(kw["bond_orders"])].tolist() == model.order2


def test_rules_overrides():
    r = analyze.ValenceRules(["C", "Xx", "S"], [0, 2], allowed={("Xx", 0): (2, 7), ("Xx", 2): (0,), ("C", 2): (2,),
                                                                ("S", 2): (4,), ("S", 0): (6, 2)},
                             masses={"Xx": 5000, "C": 13003, "H": 2014}, bond_orders=(3, 1.5, 1, 1, 2),
                             imp_H=[3, 0], device=None)
    assert r.valences == {("C", 0): (4,), ("C", 2): (2,), ("Xx", 0): (2, 7), ("Xx", 2): (0,), ("S", 0): (2, 6),
                          ("S", 2): (4,)}
    assert r.mask_table.tolist() == [[16, 4], [132, 1], [68, 16]] and r.mass_table.tolist() == [13003, 5000, 32060]
    assert r.mass_h == 2014 and r.h_type == -1 and r.groups == (3, 2, 2) and r.imp_H == [3, 0]
    assert {k: v.tolist() for k, v in r.order2_tables.items()} == {5: [6, 3, 2, 2, 4]}
    assert r.device is None and r.allowed_mask is None


def test_rules_value_errors():
    ok = dict(atom_types=["C", "N"], formal_charge=[0, 1], device=None)
    new = lambda **kw: analyze.ValenceRules(**{**ok, **kw})
    with pytest.raises(ValueError, match=r"'B' with formal charge \+1"):             # group 12
        new(atom_types=["C", "B"])
    with pytest.raises(ValueError, match=r"'C' with formal charge \+2"):
        new(formal_charge=[0, 2])
    with pytest.raises(ValueError, match="no mass for element 'Xx'"):
        new(atom_types=["Xx"], allowed={("Xx", 0): (1,), ("Xx", 1): (1,)})
    with pytest.raises(ValueError, match="'Xx' with formal charge"):
        new(atom_types=["Xx"], masses={"Xx": 1})
    with pytest.raises(ValueError, match="bond order 2.5"):
        new(bond_orders=(1, 2.5))
    with pytest.raises(ValueError, match="bond types"):
        new(bond_orders=(1,) * 9)
    with pytest.raises(ValueError, match="bond types"):
        new(bond_orders=())
    with pytest.raises(ValueError, match=r"allowed\["):
        new(allowed={("C", 0): (16,)})
    with pytest.raises(ValueError, match=r"allowed\["):
        new(allowed={"C": (4,)})
    with pytest.raises(ValueError, match="must not be empty"):
        new(atom_types=[])
    with pytest.raises(ValueError, match="must not be empty"):
        new(imp_H=[])
    with pytest.raises(ValueError, match="hydrogen counts"):
        new(imp_H=[0, -1])
    with pytest.raises(ValueError, match="bond_orders is required for 5 bond types"):
        new().order2(5)
    with pytest.raises(ValueError, match="hold 2 bond orders"):
        new(bond_orders=(1, 2)).order2(3)
    with pytest.raises(RuntimeError, match="no\\s+CPU fallback"):
        new(device="cpu")


# ---- binding and boundary --------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    assert re.search(r"^int\s+gi_mol_valence\s*\(", hdr, flags=re.M)
    assert "gi_mol_valence" in L.SIGNATURES and hasattr(lib, "gi_mol_valence")
    decl = re.search(r"^int\s+gi_mol_valence\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(L.SIGNATURES["gi_mol_valence"][1]) == len(decl.split(",")) == 30
    for name, value in (("EMPTY", 128), ("SELF_LOOP", 256), ("OVER", 512), ("FRAGMENTS", 1024), ("AROMATIC", 2048),
                        ("H_MISMATCH", 4096), ("DESC", 6), ("COUNTS", 4), ("SCRATCH", 4)):
        assert re.search(rf"#define\s+GI_VAL_{name}\s+{value}\b", hdr) and getattr(L, "VAL_" + name) == value
        assert getattr(VM, "VAL_" + name, value) == value
    assert VM.MALFORMED == analyze.MALFORMED_BITS == 1 | 2 | 8 | 16 | 32 | 64
    assert analyze.INVALID_BITS == VM.MALFORMED | 128 | 256 | 512
    assert set(analyze.VALIDITY_STATUS_MESSAGES) == {1, 2, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096}
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # an added entry point is compatible
    assert re.search(r"#define\s+GI_ABI_VERSION\s+18\b", hdr)
    assert "gi_valence.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    assert "getenv" not in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_valence.hip")).read()
    assert "gi_mol_valence" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(analyze.MoleculeValidity.DESC_NAMES) == L.VAL_DESC and analyze.MoleculeValidity.DESC_NAMES == VM.DESC
    # argument checks that need no device: nothing is launched, nothing is written, for any of these
    def call(G=0, N=13, Fn=8, Fe=3, dtype=0, nb=1, A=5, C=3, H=0, h_type=-1, term_dtype=1):
        return lib.gi_mol_valence(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, None, None, None, h_type,
                                  1008, None, term_dtype, 0, None, None, None, None, None, None, None, None, None)
    assert call() == 0                                                     # an empty batch: no launch
    assert call(G=1) == -1                                                 # no buffers
    assert call(N=129) == -1 and call(N=0) == -1 and call(Fe=9) == -1 and call(G=-1) == -1 and call(Fn=513) == -2
    assert call(dtype=2) == -1 and call(nb=2) == -1 and call(term_dtype=2) == -1
    assert call(A=6) == -1 and call(H=1) == -1 and call(A=0) == -1 and call(h_type=5) == -1 and call(h_type=-2) == -1
    assert analyze.MoleculeValidity.nbytes(0, 13) == 16 and analyze.MoleculeValidity.nbytes(3, 5) == 16 + 108 + 30


def test_python_boundary_raises():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    host_rules = analyze.ValenceRules(device=None, **RULE_ARGS["gdb13"])
    for call in (lambda: analyze.validity(n, e, None, host_rules), lambda: analyze.fraction_valid(n, e, None, host_rules)):
        with pytest.raises(RuntimeError, match="no CPU"):                  # CPU tensors
            call()
    with pytest.raises(TypeError, match="tensor"):
        analyze.validity(n.numpy(), e.numpy(), None, host_rules)
    with pytest.raises(TypeError, match="ValenceRules"):
        analyze.validity(n, e, None, [5, 3])
    with pytest.raises(RuntimeError, match="no\\s+CPU fallback"):
        analyze.ValenceRules(device="cpu", **RULE_ARGS["gdb13"])
    if not torch.cuda.is_available():
        return
    dn, de, dk = n.cuda(), e.cuda(), torch.zeros(2, dtype=torch.int8).cuda()   # raised before anything is launched
    rules = analyze.ValenceRules(**RULE_ARGS["gdb13"])
    with pytest.raises(RuntimeError, match="device=None"):
        analyze.validity(dn, de, None, host_rules)
    with pytest.raises(ValueError, match="contiguous"):
        analyze.validity(dn, de.transpose(1, 2), None, rules)
    with pytest.raises(TypeError, match="float32 or both int8"):
        analyze.validity(dn.float(), de, None, rules)
    with pytest.raises(ValueError, match="does not match"):
        analyze.validity(dn, de[:, :12], None, rules)
    with pytest.raises(ValueError, match="nodes must be"):
        analyze.validity(dn[0], de, None, rules)
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.validity(dn, de, torch.zeros(2, dtype=torch.int8), rules)
    with pytest.raises(TypeError, match="n_nodes"):
        analyze.validity(dn, de, dk.float(), rules)
    with pytest.raises(ValueError, match="do not fit"):
        analyze.validity(dn[:, :, :7].contiguous(), de, None, rules)
    with pytest.raises(ValueError, match="bond_orders is required"):
        analyze.validity(dn, de[..., :2].contiguous(), None, rules)
    with pytest.raises(RuntimeError, match="termination"):
        analyze.validity(dn, de, None, rules, termination=torch.zeros(2))
    with pytest.raises(ValueError, match="termination"):
        analyze.validity(dn, de, None, rules, termination=torch.zeros(3, device="cuda"))
