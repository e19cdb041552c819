"""CPU: the specification of the molecule strings (tests/smiles_model.py: writer, independent reader, graph comparison),
``analyze.write_smi``, and the binding and Python boundary of ``analyze.smiles`` (gi_mol_smiles).  No device compute is
issued.

The writer is pinned to strings worked out by hand; the reader to the 30 SMILES strings that RDKit wrote for the
reference's shipped molecules (tests/golden/golden_valence.npz), which neither the writer nor the reader produced;
writer and reader to each other by the round trip over every fixture molecule.  The strings are a spelling of the
labelled graph, NOT RDKit's canonical SMILES: no parity with RDKit is claimed (there is no RDKit to compare with)."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd.analyze import MoleculeStrings, smiles, write_smi      # the feature under test
from graphinvent_amd import lib as L
from tests import canon_model as CM
from tests import smiles_model as SM
from tests import valence_model as VM
from tests.test_valence_cpu import RULE_ARGS, model_of, model_rules, shipped, stored_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("gdb13", "arom5", "chiral6", "atoms_charges", "imp_h_chirality")
#: per fixture set: molecules with a string, and molecules left out (malformed, empty, self-looped or aromatic by
#: tests/valence_model.py).  arom5 and chiral6 are mostly aromatic; half of the generated sets' slots are empty graphs.
COVERED = {"gdb13": (140, 0), "arom5": (3, 17), "chiral6": (1, 11), "atoms_charges": (32, 32),
           "imp_h_chirality": (33, 47)}
_CACHE = {}


def ring_number(k):
    return str(k) if k < 10 else f"%{k}"


def hand_cases():
    """name -> dict(rules, nodes, edges, n, kw, text, status, length): molecules whose strings are worked out by hand.
    ``n`` is None where the leading non-empty rows say it."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    C, O, N_, F, S = ("C", 0), ("O", 0), ("N", 0), ("F", 0), ("S", 0)
    cases = {}

    def add(name, atoms, bonds, text, status=0, N=8, rules="chem", length=None, n=None, **kw):
        nodes, edges = VM.molecule(N, model_rules(rules), atoms, bonds)
        cases[name] = dict(rules=rules, nodes=nodes, edges=edges, n=n, kw=kw, text=text, status=status,
                           length=len(text) if length is None else length)

    add("methane", [C], [], "C")
    add("ethanol", [C, C, O], [(0, 1, 1), (1, 2, 1)], "CCO")
    add("acetic_acid", [C, C, O, O], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], "CC(=O)O")
    add("benzene", [C] * 6, [(i, (i + 1) % 6, 2 - i % 2) for i in range(6)], "C1=CC=CC=C1")
    add("acetonitrile", [C, C, N_], [(0, 1, 1), (1, 2, 3)], "CC#N")
    add("ammonium", [("N", 1)], [], "[NH4+]")
    add("alkoxide", [C, ("O", -1)], [(0, 1, 1)], "C[O-]")
    add("nitro", [C, ("N", 1), O, ("O", -1)], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], "C[N+](=O)[O-]")
    add("sf6", [S] + [F] * 6, [(0, i, 1) for i in range(1, 7)], "S(F)(F)(F)(F)(F)F")
    add("five_bonded_c", [C] + [F] * 5, [(0, i, 1) for i in range(1, 6)], "C(F)(F)(F)(F)F", SM.SMI_OVER)
    add("two_components", [C, O], [], "C.O", SM.SMI_FRAGMENTS)
    # an explicit hydrogen atom, a proton, a chloride, an oxonium, a carbanion with its two hydrogens
    add("hydrogen_cyanide", [("H", 0), C, N_], [(0, 1, 1), (1, 2, 3)], "[H]C#N")
    add("proton", [("H", 1)], [], "[H+]")
    add("chloride", [("Cl", -1)], [], "[Cl-]")
    add("oxonium", [("O", 1), C, C, C], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], "[O+](C)(C)C")
    add("carbanion", [("C", -1), C], [(0, 1, 1)], "[CH2-]C")
    # spiro[2.2]pentane from the spiro atom: two openings at one atom
    add("spiro", [C] * 5, [(0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 3, 1), (3, 4, 1), (4, 0, 1)], "C12(CC1)CC2")
    # bicyclo[2.2.0]hexane from a fusion atom: 0-1 shared, 0-2-3-1 and 0-4-5-1
    add("fused", [C] * 6, [(0, 1, 1), (0, 2, 1), (2, 3, 1), (3, 1, 1), (0, 4, 1), (4, 5, 1), (5, 1, 1)],
        "C12C(CC1)CC2")
    # cubane, bottom 0-1-2-3, top 4-5-6-7: walked 0 1 2 3 7 4 5 6; four numbers open at atom 2, number 1 reused at 7
    cube = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1), (4, 5, 1), (5, 6, 1), (6, 7, 1), (7, 4, 1)] + \
           [(i, i + 4, 1) for i in range(4)]
    add("cubane", [C] * 8, cube, "C12C3C4C1C1C2C3C41")
    # a 2 x 12 ladder numbered rail by rail: walked along rail 0..11, over the last rung, back along 23..12
    ladder = [(i, i + 1, 1) for i in range(11)] + [(12 + i, 13 + i, 1) for i in range(11)] + \
             [(i, 12 + i, 1) for i in range(12)]
    add("ladder", [C] * 24, ladder, "".join("C" + ring_number(k) for k in range(1, 12)) + "CC" +
        "".join("C" + ring_number(k) for k in range(11, 0, -1)), N=24)
    # a 127-atom path whose 128th atom is bonded to atoms 0 .. 125: 125 ring bonds are open when it is reached
    add("ring_limit", [C] * 128, [(i, i + 1, 1) for i in range(126)] + [(127, i, 1) for i in range(126)], "",
        SM.SMI_RING_LIMIT | SM.SMI_OVER, N=128)
    add("empty", [], [], "", SM.SMI_EMPTY)
    add("aromatic", [("C", 0, 1)] * 6, [(i, (i + 1) % 6, 1.5) for i in range(6)], "", SM.SMI_AROMATIC, N=13,
        rules="arom5", hydrogens="fill")
    add("truncated", [C] * 20, [(i, i + 1, 1) for i in range(19)], "", SM.SMI_TRUNCATED, N=24, length=20, max_len=16)
    add("fits_exactly", [C] * 16, [(i, i + 1, 1) for i in range(15)], "C" * 16, N=24, max_len=16)
    add("self_loop", [C, C], [(0, 1, 1)], "", SM.SMI_SELF_LOOP)
    cases["self_loop"]["edges"][1, 1, 0] = 1
    add("asymmetric", [C, C, O], [(0, 1, 1), (1, 2, 1)], "", VM.MOL_ASYMMETRIC)
    cases["asymmetric"]["edges"][0, 2, 0] = 1
    add("multi_bond", [C, C, O], [(0, 1, 1), (1, 2, 1)], "", VM.MOL_MULTI_BOND)
    cases["multi_bond"]["edges"][0, 1, 1] = cases["multi_bond"]["edges"][1, 0, 1] = 1
    # stored hydrogens that differ from the fill: brackets carry them (methanol stored as CH3-O without its H)
    add("stored_h", [("C", 0, 3), ("O", 0, 0)], [(0, 1, 1)], "C[O]", N=13, rules="arom5", hydrogens="stored")
    add("stored_h_filled", [("C", 0, 3), ("O", 0, 0)], [(0, 1, 1)], "CO", N=13, rules="arom5", hydrogens="fill")
    add("stored_h2", [("C", 0, 2), ("N", 0, 2)], [(0, 1, 1)], "[CH2]N", N=13, rules="arom5")
    _CACHE["hand"] = cases
    return cases


def grouped(cases):
    """The hand cases as batches of equal shape and arguments: [(names, rules name, nodes, edges, kw)]."""
    groups = {}
    for name, c in cases.items():
        key = (c["rules"], c["nodes"].shape, tuple(sorted(c["kw"].items())))
        groups.setdefault(key, []).append(name)
    return [(names, key[0], np.stack([cases[k]["nodes"] for k in names]), np.stack([cases[k]["edges"] for k in names]),
             dict(key[2])) for key, names in groups.items()]


def canon_of(golden_dir, c):
    """tests/canon_model.canonical of a fixture set, computed once and shared (read only)."""
    if ("canon", c) not in _CACHE:
        nodes, edges, n, _ = stored_set(golden_dir, c)
        _CACHE[("canon", c)] = CM.canonical(nodes, edges, n)
    return _CACHE[("canon", c)]


def strings_of(golden_dir, c, ranked=False, hydrogens=None):
    """The model's batch result on a fixture set, in input order or with the canon model's rank; computed once."""
    key = ("strings", c, ranked, hydrogens)
    if key not in _CACHE:
        nodes, edges, n, _ = stored_set(golden_dir, c)
        rank = canon_of(golden_dir, c)["rank"] if ranked else None
        _CACHE[key] = SM.write_batch(nodes, edges, n, model_rules(c), rank=rank, hydrogens=hydrogens)
    return _CACHE[key]


def left_out(golden_dir, c):
    """The molecules that may have an empty string, by the VALENCE model (never by the writer's own status)."""
    status = model_of(golden_dir, c)["status"]
    return (status & (VM.MALFORMED | VM.VAL_EMPTY | VM.VAL_SELF_LOOP | VM.VAL_AROMATIC)) != 0


# ---- the reader against the reference's data ----------------------------------------------------------------------

def test_reader_on_the_shipped_smiles(golden_dir):
    nodes, edges, V = shipped(golden_dir)
    strings = [str(s) for split in V["splits"] for s in V[f"{split}::smiles"]]
    assert len(strings) == 30 == len(nodes) and strings[0] == "CC1C2N1CC1=C2CC=C1"
    r = model_rules("gdb13")
    assert not VM.validity(nodes, edges, None, r)["status"].any()            # the left-out set is empty
    for k, s in enumerate(strings):
        got, want = SM.read(s), SM.graph_of(nodes[k], edges[k], None, r)
        assert SM.same(got, want), (k, s, got, want)
    assert sum(SM.read(s)["hydrogens"][0] for s in strings) > 0              # hydrogens are compared, and there are some


def test_reader_on_hand_strings():
    g = SM.read("C[N+](=O)[O-]")
    assert g == dict(elements=["C", "N", "O", "O"], charges=[0, 1, 0, -1], hydrogens=[3, 0, 0, 0],
                     bonds={(0, 1): 1, (1, 2): 2, (1, 3): 1})
    g = SM.read("C1=CC=CC=C1")
    assert g["hydrogens"] == [1] * 6 and g["bonds"][(0, 5)] == 1 and sorted(g["bonds"].values()) == [1, 1, 1, 2, 2, 2]
    g = SM.read("C%12CC%12.[NH4+].[ClH2+2].S(F)(F)(F)(F)(F)F.N(=O)(=O)C.Cl.BrC#N")
    assert g["bonds"][(0, 2)] == 1 and g["elements"][3:5] == ["N", "Cl"] and g["hydrogens"][3:5] == [4, 2]
    assert g["charges"][3:5] == [1, 2] and g["hydrogens"][5] == 0 and g["hydrogens"][12] == 0   # S at 6, N at 5
    assert g["elements"][-4:] == ["Cl", "Br", "C", "N"] and g["hydrogens"][-4:] == [1, 0, 0, 0]
    assert SM.read("C=1CC=1")["bonds"][(0, 2)] == 2 and SM.read("[H]C#N")["hydrogens"] == [0, 0, 0]
    for bad in ("C1CC", "C(C", "CC)", "C=", "[CH", "c1ccccc1", "C..C", "C11", "=C", "C%1C", "[C@H](F)(Cl)Br", "Xe"):
        with pytest.raises(SM.SmilesError):
            SM.read(bad)
    a, b = SM.read("OCC"), SM.read("CCO")
    assert SM.same(a, b) and not SM.same(a, SM.read("CC=O")) and not SM.same(a, SM.read("CC[O-]"))
    assert not SM.same(SM.read("C[O]"), SM.read("CO")) and not SM.same(SM.read("CCC"), SM.read("C1CC1"))


# ---- the writer: exact strings ---------------------------------------------------------------------------------

def test_writer_on_hand_cases():
    cases = hand_cases()
    for name, c in cases.items():
        r = model_rules(c["rules"])
        got = SM.write(c["nodes"], c["edges"], c["n"], r, **c["kw"])
        assert got["text"].decode() == c["text"], (name, got["text"])
        assert got["status"] == c["status"] and got["length"] == c["length"], (name, got["status"], got["length"])
        if c["text"]:
            n = CM.derived_n(c["nodes"])
            pos = got["atom_pos"]
            assert (pos[n:] == -1).all() and (pos[:n] >= 0).all() and len(set(pos[:n].tolist())) == n, name
            assert SM.same(SM.read(c["text"]), SM.graph_of(c["nodes"], c["edges"], c["n"], r, c["kw"].get("hydrogens"))), name
        else:
            assert (got["atom_pos"] == -1).all(), name
    assert "%10" in cases["ladder"]["text"] and "%11" in cases["ladder"]["text"] and len(cases["ladder"]["text"]) == 54
    pos = SM.write(cases["acetic_acid"]["nodes"], cases["acetic_acid"]["edges"], None, model_rules("chem"))["atom_pos"]
    assert pos[:4].tolist() == [0, 1, 4, 6]                                   # CC(=O)O: the token, not the bond symbol
    pos = SM.write(cases["nitro"]["nodes"], cases["nitro"]["edges"], None, model_rules("chem"))["atom_pos"]
    assert pos[:4].tolist() == [0, 1, 7, 9]                                   # C[N+](=O)[O-]
    assert SM.default_max_len(13) == 160 and SM.default_max_len(128) == 1552 and SM.default_max_len(1) == 16


def test_writer_follows_the_rank():
    c = hand_cases()["ethanol"]
    r = model_rules("chem")
    for rank, want, pos in (([2, 1, 0], "OCC", [2, 1, 0]), ([1, 0, 2], "C(C)O", [2, 0, 4]), ([5, 5, 5], "CCO", [0, 1, 2]),
                            ([0, 7, -3], "OCC", [2, 1, 0])):
        got = SM.write(c["nodes"], c["edges"], None, r, rank=np.array(rank + [-1] * 5, np.int32))
        assert got["text"].decode() == want and got["atom_pos"][:3].tolist() == pos, (rank, got)
    two = hand_cases()["two_components"]
    got = SM.write(two["nodes"], two["edges"], None, r, rank=np.array([1, 0] + [-1] * 6, np.int32))
    assert got["text"] == b"O.C" and got["status"] == SM.SMI_FRAGMENTS


# ---- the round trip over the fixture sets ---------------------------------------------------------------------------

@pytest.mark.parametrize("c", SETS)
def test_round_trip_on_the_fixture_sets(golden_dir, c):
    nodes, edges, n, _ = stored_set(golden_dir, c)
    r = model_rules(c)
    out = left_out(golden_dir, c)
    assert (int((~out).sum()), int(out.sum())) == COVERED[c]
    for ranked in (False, True):
        res = strings_of(golden_dir, c, ranked)
        for g in range(len(nodes)):
            s = res["strings"][g]
            if not s:
                assert out[g], (c, ranked, g, res["status"][g])              # only those may have no string
                continue
            assert not out[g] and res["length"][g] == len(s)
            want = SM.graph_of(nodes[g], edges[g], None if n is None else n[g], r)
            assert SM.same(SM.read(s), want), (c, ranked, g, s)
    if c == "gdb13":
        assert not out.any()


@pytest.mark.parametrize("c", SETS)
def test_hydrogen_fill_round_trips_too(golden_dir, c):
    if not model_rules(c).groups[2]:
        return                                                               # no implicit-H segment: "fill" is the default
    nodes, edges, n, _ = stored_set(golden_dir, c)
    res = strings_of(golden_dir, c, False, "fill")
    for g, s in enumerate(res["strings"]):
        if s:
            want = SM.graph_of(nodes[g], edges[g], None if n is None else n[g], model_rules(c), "fill")
            assert SM.same(SM.read(s), want), (c, g, s)


# ---- canonical strings ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SETS)
def test_canonical_strings_do_not_depend_on_the_node_order(golden_dir, c):
    nodes, edges, n, _ = stored_set(golden_dir, c)
    r = model_rules(c)
    base = strings_of(golden_dir, c, True)
    canon = canon_of(golden_dir, c)
    rng = np.random.default_rng(11)
    for g in range(len(nodes)):
        if not base["strings"][g]:
            continue
        k = int(VM.judge(nodes[g], edges[g], None if n is None else n[g], r)["desc"][0])
        for _ in range(8):
            perm = rng.permutation(k)
            pn, pe = CM.permute(nodes[g], edges[g], perm)
            rank = np.full(len(pn), -1, np.int32)
            rank[CM.canonical_order(pn, pe, k)] = np.arange(k)
            got = SM.write(pn, pe, k, r, rank=rank)
            assert got["text"].decode() == base["strings"][g], (c, g, perm)
    # equal strings exactly when equal canonical keys, among the molecules that have a string
    have = [g for g in range(len(nodes)) if base["strings"][g]]
    by_string, by_key = {}, {}
    for g in have:
        by_string.setdefault(base["strings"][g], []).append(g)
        by_key.setdefault(tuple(canon["key"][g].tolist()), []).append(g)
    assert sorted(by_string.values()) == sorted(by_key.values()), c


# ---- write_smi --------------------------------------------------------------------------------------------------

def test_write_smi_reads_back_row_for_row(tmp_path, golden_dir):
    res = strings_of(golden_dir, "atoms_charges")
    strings = res["strings"]
    valid = model_of(golden_dir, "atoms_charges")["valid"]
    path = tmp_path / "generated.smi"
    replaced = write_smi(str(path), strings, valid=valid)
    header, rows = SM.read_smi(str(path))
    assert header == "SMILES Name" and len(rows) == len(strings)             # the shipped files' header row
    holes = [k for k, s in enumerate(strings) if not s or not valid[k]]
    assert replaced == len(holes) and 0 < len(holes) < len(strings)
    assert any(strings[k] and not valid[k] for k in holes) and any(not strings[k] for k in holes)
    for k, (s, name) in enumerate(rows):
        assert name == str(k)
        if k in holes:
            assert s == "[Xe]"
        else:
            assert s == strings[k] and SM.same(SM.read(s), SM.read(strings[k]))
    write_smi(str(path), ["CCO", "", "C"], placeholder="*")
    assert open(path).read() == "SMILES Name\nCCO 0\n* 1\nC 2\n"
    write_smi(str(path), ["CCO", "C"], valid=torch.tensor([0.0, 1.0]))
    assert open(path).read() == "SMILES Name\n[Xe] 0\nC 1\n"
    with pytest.raises(ValueError, match="validity entries"):
        write_smi(str(path), ["C"], valid=[1, 1])
    with pytest.raises(ValueError, match="placeholder"):
        write_smi(str(path), ["C"], placeholder="a b")


# ---- binding and boundary --------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    decl = re.search(r"^int\s+gi_mol_smiles\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(L.SIGNATURES["gi_mol_smiles"][1]) == len(decl.split(",")) == 25 and hasattr(lib, "gi_mol_smiles")
    for name, value in (("EMPTY", 128), ("SELF_LOOP", 256), ("OVER", 512), ("FRAGMENTS", 1024), ("AROMATIC", 2048),
                        ("RING_LIMIT", 8192), ("TRUNCATED", 16384), ("MAX_LEN", 8192)):
        assert re.search(rf"#define\s+GI_SMI_{name}\s+{value}\b", hdr) and getattr(L, "SMI_" + name) == value
        assert getattr(SM, "SMI_" + name) == value
    assert (L.SMI_EMPTY, L.SMI_SELF_LOOP, L.SMI_OVER, L.SMI_FRAGMENTS, L.SMI_AROMATIC) == \
        (L.VAL_EMPTY, L.VAL_SELF_LOOP, L.VAL_OVER, L.VAL_FRAGMENTS, L.VAL_AROMATIC)
    assert set(analyze.SMILES_STATUS_MESSAGES) == {1, 2, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 8192, 16384}
    assert analyze.NO_STRING_BITS == SM.NO_STRING | SM.SMI_TRUNCATED
    assert "gi_smiles.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_smiles.hip")).read()
    assert "getenv" not in src and "hipMemset" not in src                  # nothing is cleared in front of the launch
    assert analyze.default_smiles_len(13) == SM.default_max_len(13) and analyze.default_smiles_len(128) == 1552
    # the LDS budget at the limits: rows of N = 128, Fe = 8, the string and the ring text, and the static arrays
    assert 8 * 128 * 16 + 2 * L.SMI_MAX_LEN + 24 * 1024 <= 64 * 1024
    lay = MoleculeStrings.layout(3, 5, 32)
    assert lay["text"][:2] == (0, 96) and lay["length"][0] == 96 and lay["atom_pos"] == (120, 60, "int32", (3, 5))
    # argument checks that need no device: nothing is launched, nothing is written, for any of these
    def call(G=0, N=13, Fn=8, Fe=3, dtype=0, nb=1, A=5, C=3, H=0, stored=0, max_len=160):
        return lib.gi_mol_smiles(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, None, None, None, None,
                                 stored, None, max_len, None, None, None, None, None)
    assert call() == 0                                                     # an empty batch: no launch
    assert call(G=1) == -1                                                 # no buffers
    assert call(N=129) == -1 and call(N=0) == -1 and call(Fe=9) == -1 and call(G=-1) == -1 and call(Fn=513) == -2
    assert call(dtype=2) == -1 and call(nb=2) == -1 and call(A=6) == -1 and call(A=0) == -1
    assert call(stored=1) == -1 and call(stored=2) == -1 and call(Fn=9, H=1, stored=1) == 0
    assert call(max_len=0) == -1 and call(max_len=24) == -1 and call(max_len=8192) == 0 and call(max_len=8208) == -2


def test_python_boundary_raises():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    host_rules = analyze.ValenceRules(device=None, **RULE_ARGS["gdb13"])
    with pytest.raises(RuntimeError, match="no CPU"):                       # CPU tensors
        smiles(n, e, None, host_rules)
    with pytest.raises(TypeError, match="ValenceRules"):
        smiles(n, e, None, [5, 3])
    with pytest.raises(ValueError, match="not both"):
        smiles(n, e, None, host_rules, rank=torch.zeros(2, 13, dtype=torch.int32), canonical=True)
    with pytest.raises(ValueError, match="'fill' or 'stored'"):
        smiles(n, e, None, host_rules, hydrogens="none")
    with pytest.raises(ValueError, match="implicit-H segment"):
        smiles(n, e, None, host_rules, hydrogens="stored")
    for bad in ("Xx1", "C-", "", "Uuo", "É"):
        rules = analyze.ValenceRules(["C", bad], [0], allowed={(bad, 0): (1,)}, masses={bad: 1}, device=None)
        with pytest.raises(ValueError, match="one or two ASCII letters"):
            smiles(n, e, None, rules)
    assert analyze.symbol_table(["C", "Cl", "Xx"]).tolist() == [[67, 0], [67, 108], [88, 120]]
    if not torch.cuda.is_available():
        return
    dn, de = n.cuda(), e.cuda()                                              # raised before anything is launched
    rules = analyze.ValenceRules(**RULE_ARGS["gdb13"])
    with pytest.raises(RuntimeError, match="device=None"):
        smiles(dn, de, None, host_rules)
    for bad in (0, 24, 8208, 16.0, True):
        with pytest.raises(ValueError, match="max_len"):
            smiles(dn, de, None, rules, max_len=bad)
    with pytest.raises(RuntimeError, match="rank"):
        smiles(dn, de, None, rules, rank=torch.zeros(2, 13, dtype=torch.int32))
    with pytest.raises(ValueError, match="rank"):
        smiles(dn, de, None, rules, rank=torch.zeros(2, 13, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="rank"):
        smiles(dn, de, None, rules, rank=torch.zeros(2, 12, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="do not fit"):
        smiles(dn[:, :, :7].contiguous(), de, None, rules)
    with pytest.raises(ValueError, match="bond_orders is required"):
        smiles(dn, de[..., :2].contiguous(), None, rules)
