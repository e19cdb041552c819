"""CPU: the specification of the SMILES reader (tests/smiles_read_model.py), and the binding and Python boundary of
``analyze.read_smiles`` / ``read_smi`` / ``pack_strings`` (gi_smiles_read).  No device compute is issued.

The model is pinned four ways: to the independent reader ``tests/smiles_model.py::read`` (written from the OpenSMILES
text, sharing nothing with it) on every string that reader accepts; to the writer's model ``smiles_model.write`` as its
exact inverse, byte for byte; to the reference's 979 GDB-13 training strings, all of which must read; and to one
hand-made string per status bit.  NO aromatic input and NO stereo: those strings must get their bit, not a molecule."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd.analyze import ReadMolecules, pack_strings, read_smi, read_smiles     # the feature under test
from graphinvent_amd import lib as L
from tests import smiles_model as SM
from tests import smiles_read_model as RM
from tests import valence_model as VM
from tests.test_smiles_cpu import SETS, hand_cases, strings_of
from tests.test_valence_cpu import RULE_ARGS, model_rules, shipped, stored_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: the strings of tests/test_smiles_cpu.py::test_reader_on_hand_strings, the accepted and the refused ones
HAND_STRINGS = ("C[N+](=O)[O-]", "C1=CC=CC=C1", "C%12CC%12.[NH4+].[ClH2+2].S(F)(F)(F)(F)(F)F.N(=O)(=O)C.Cl.BrC#N",
                "C=1CC=1", "[H]C#N", "OCC", "CCO", "CC=O", "CC[O-]", "C[O]", "CO", "CCC", "C1CC1")
BAD = ("C1CC", "C(C", "CC)", "C=", "[CH", "c1ccccc1", "C..C", "C11", "=C", "C%1C", "[C@H](F)(Cl)Br", "Xe")
#: the GDB-13 1K set's preprocessing_params.csv: atom_types, formal_charge, imp_H, max_n_nodes; no aromatic bonds
GDB13_ARGS = dict(atom_types=["C", "N", "O", "S", "Cl"], formal_charge=[-1, 0, 1], imp_H=[0, 1, 2, 3])
GDB13_N = 13
_CACHE = {}


def wide_rules():
    """Rules that hold everything the hand-made strings say: every organic element, H, charges up to +2, stored
    hydrogen counts 0 .. 6 (so that ``graph_of`` compares the counts the string states, not a fill)."""
    if "wide" not in _CACHE:
        types = ["B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I", "H"]
        charges = [-1, 0, 1, 2]
        _CACHE["wide"] = VM.Rules(types, charges, imp_H=list(range(7)),
                                  allowed={(a, q): tuple(range(1, 8)) for a in types for q in charges
                                           if VM.valences_of(a, q) is None})
    return _CACHE["wide"]


def gdb13_strings(golden_dir):
    if "gdb13_1K" not in _CACHE:
        header, rows = SM.read_smi(os.path.join(golden_dir, "smiles_read_gdb13_1K.smi"))
        assert header == "SMILES Name"
        _CACHE["gdb13_1K"] = [s for s, _ in rows], [name for _, name in rows]
    return _CACHE["gdb13_1K"]


def gdb13_model(golden_dir):
    """The model's result on the GDB-13 strings, computed once and shared (read only)."""
    if "gdb13_model" not in _CACHE:
        _CACHE["gdb13_model"] = RM.read_batch(gdb13_strings(golden_dir)[0], None, VM.Rules(**GDB13_ARGS), GDB13_N)
    return _CACHE["gdb13_model"]


def read_string(s, rules, N, **kw):
    text, length = RM.pack([s])
    return RM.read_one(text[0], int(length[0]), rules, N, sum(rules.groups) + kw.pop("n_chirality", 0),
                       len(rules.order2), **kw)


def status_cases():
    """name -> (string, rules name or Rules, N, keywords, the status expected): one hand-made string per status bit,
    and the neighbours that must NOT set it."""
    gdb = VM.Rules(**GDB13_ARGS)
    single_double = VM.Rules(["C", "N"], [0], bond_orders=(1, 2))
    return {
        "empty": ("", gdb, 4, {}, RM.RD_EMPTY),
        "unclosed_branch": ("C(C", gdb, 4, {}, RM.RD_SYNTAX),
        "unclosed_bracket": ("C[CH", gdb, 4, {}, RM.RD_SYNTAX),
        "dangling_bond": ("C=", gdb, 4, {}, RM.RD_SYNTAX),
        "bond_without_atom": ("=C", gdb, 4, {}, RM.RD_SYNTAX),
        "digit_without_atom": ("1CC1", gdb, 4, {}, RM.RD_SYNTAX),
        "dot_dot": ("C..C", gdb, 4, {}, RM.RD_SYNTAX),
        "unknown_byte": ("C!C", gdb, 4, {}, RM.RD_SYNTAX),
        "percent_one_digit": ("C%1C", gdb, 4, {}, RM.RD_SYNTAX),
        "bare_h": ("HC", gdb, 4, {}, RM.RD_SYNTAX),
        "empty_branch": ("C()C", gdb, 4, {}, RM.RD_SYNTAX),
        "ring_open": ("C1CC", gdb, 4, {}, RM.RD_RING_OPEN),
        "ring_order": ("C=1CC#1", gdb, 4, {}, RM.RD_RING_ORDER),
        "ring_to_itself": ("C11", gdb, 4, {}, RM.RD_SELF_LOOP),
        "pair_twice": ("C12CC12", gdb, 4, {}, RM.RD_MULTI_BOND),
        "too_many": ("CCCC(C)C", gdb, 4, {}, RM.RD_TOO_MANY),
        "element": ("C[Se]C", gdb, 4, {}, RM.RD_ELEMENT),
        "bare_element": ("CBr", gdb, 4, {}, RM.RD_ELEMENT),
        "charge": ("C[N+2]", gdb, 4, {}, RM.RD_CHARGE),
        "h_count": ("[CH5]", gdb, 4, {}, RM.RD_HCOUNT),
        "bond_order": ("C#N", single_double, 4, {}, RM.RD_BOND_ORDER),
        "aromatic": ("c1ccccc1", gdb, 13, {}, RM.RD_AROMATIC),
        "aromatic_bracket": ("C[nH]C", gdb, 13, {}, RM.RD_AROMATIC),
        "aromatic_bond": ("C:C", gdb, 13, {}, RM.RD_AROMATIC),
        "stereo_bond": ("F/C=C/F", "chem", 4, {}, RM.RD_STEREO),
        "stereo_atom": ("[C@H](F)(Cl)Br", "wide", 4, {}, RM.RD_STEREO),
        "stereo_bond_dropped": ("F/C=C\\F", "chem", 4, dict(drop_stereo=True), RM.RD_STEREO_DROPPED),
        "stereo_atom_dropped": ("[C@@H](F)(Cl)Br", "wide", 4, dict(drop_stereo=True), RM.RD_STEREO_DROPPED),
        "isotope": ("[13CH4]", gdb, 4, {}, RM.RD_UNSUPPORTED),
        "atom_class": ("[CH3:1]C", gdb, 4, {}, RM.RD_UNSUPPORTED),
        "plus_plus": ("[N++]", gdb, 4, {}, RM.RD_UNSUPPORTED),
        "quadruple": ("C$C", gdb, 4, {}, RM.RD_UNSUPPORTED),
        "wildcard": ("C*", gdb, 4, {}, RM.RD_UNSUPPORTED),
        "over": ("C(F)(F)(F)(F)F", "chem", 8, {}, RM.RD_OVER),
        "fragments": ("CC.O", gdb, 4, {}, RM.RD_FRAGMENTS),
        "ring_across_the_dot": ("C1.C1", gdb, 4, {}, 0),
        "exactly_n": ("CCCC", gdb, 4, {}, 0),
        "ring_bond_on_one_end": ("C=1CC1", gdb, 4, {}, 0),
    }


def rules_of(r):
    return wide_rules() if r == "wide" else model_rules(r) if isinstance(r, str) else r


# ---- 1: the model against the independent reader ------------------------------------------------------------------

def strings_to_compare(golden_dir):
    """[(string, rules, N, hydrogens for graph_of)]: every string of the three sources."""
    out = [(s, wide_rules(), 24, "stored") for s in HAND_STRINGS + BAD]
    out += [(c["text"], wide_rules(), len(c["nodes"]), "stored") for c in hand_cases().values() if c["text"]]
    nodes, _, V = shipped(golden_dir)
    out += [(str(s), model_rules("gdb13"), nodes.shape[1], None) for split in V["splits"] for s in V[f"{split}::smiles"]]
    for c in SETS:
        N = stored_set(golden_dir, c)[0].shape[1]
        for ranked in (False, True):
            out += [(s, model_rules(c), N, None) for s in strings_of(golden_dir, c, ranked)["strings"] if s]
    return out


def test_model_agrees_with_the_independent_reader(golden_dir):
    accepted = refused = 0
    for s, rules, N, hydrogens in strings_to_compare(golden_dir):
        try:
            want = SM.read(s)
        except SM.SmilesError:
            refused += 1
            continue
        accepted += 1
        got = read_string(s, rules, N)
        assert not got["status"] & RM.RD_ERROR, (s, got["status"])
        graph = SM.graph_of(got["nodes"], got["edges"], int(got["n_nodes"]), rules, hydrogens)
        assert graph == want and SM.same(graph, want), (s, graph, want)     # atom for atom: both number in string order
    assert refused == len(BAD) and accepted > 400
    for s in BAD:                                                           # what that reader refuses gets an error bit
        got = read_string(s, wide_rules(), 24)
        assert got["status"] & RM.RD_ERROR and got["n_nodes"] == 0 and not got["nodes"].any(), (s, got["status"])
    assert read_string("Xe", wide_rules(), 24)["status"] == RM.RD_SYNTAX
    assert read_string("c1ccccc1", wide_rules(), 24)["status"] == RM.RD_AROMATIC
    assert read_string("[C@H](F)(Cl)Br", wide_rules(), 24)["status"] == RM.RD_STEREO


# ---- 2: the exact inverse of the writer ---------------------------------------------------------------------------

@pytest.mark.parametrize("c", SETS)
def test_reader_is_the_exact_inverse_of_the_writer(golden_dir, c):
    nodes, edges, n_all, _ = stored_set(golden_dir, c)
    rules = model_rules(c)
    A, C, H = rules.groups
    N, Fn = nodes.shape[1:]
    n_chir = Fn - (A + C + H)
    done = 0
    for ranked in (False, True):
        res = strings_of(golden_dir, c, ranked)                             # hydrogens: "stored" with a segment, else "fill"
        for g, s in enumerate(res["strings"]):
            if not s:
                continue
            for none in range(max(n_chir, 1)):
                got = read_string(s, rules, N, n_chirality=n_chir, none_chirality=none)
                n = int(got["n_nodes"])
                assert not got["status"] & RM.RD_ERROR and n == (res["atom_pos"][g] >= 0).sum(), (c, g, s, got["status"])
                perm = np.argsort(res["atom_pos"][g][:n], kind="stable")
                assert np.array_equal(got["atom_pos"][:n], res["atom_pos"][g][perm]) and (got["atom_pos"][n:] == -1).all()
                assert np.array_equal(got["nodes"][:n, :A + C + H], nodes[g][perm][:, :A + C + H]), (c, g, s)
                assert not got["nodes"][n:].any()
                assert np.array_equal(got["edges"][:n, :n], edges[g][perm][:, perm]) and got["edges"].sum() == edges[g].sum()
                if n_chir:
                    want = np.zeros((n, n_chir), np.int8)
                    want[:, none] = 1
                    assert np.array_equal(got["nodes"][:n, A + C + H:], want), (c, g, none)
            again = SM.write(got["nodes"], got["edges"], n, rules)
            assert again["text"].decode() == s and again["status"] == res["status"][g], (c, g, s, again["text"])
            done += 1
    assert done > 0
    if H:                                                                   # the other hydrogen count: the text round trip
        fill = strings_of(golden_dir, c, False, "fill")
        read_back = refused = 0
        for g, s in enumerate(fill["strings"]):
            if not s:
                continue
            got = read_string(s, rules, N, n_chirality=n_chir)
            if got["status"] & RM.RD_ERROR:
                assert got["status"] & RM.RD_ERROR == RM.RD_HCOUNT, (c, g, s)   # a fill the stored table does not hold
                refused += 1
                continue
            assert SM.write(got["nodes"], got["edges"], int(got["n_nodes"]), rules, hydrogens="stored")["text"].decode() == s
            read_back += 1
        assert read_back + refused == sum(1 for s in fill["strings"] if s) and (read_back > 0 or c == "chiral6")


# ---- 3: the reference's GDB-13 strings ------------------------------------------------------------------------------

def test_all_gdb13_strings_read_and_are_valid(golden_dir):
    strings, names = gdb13_strings(golden_dir)
    assert len(strings) == 979 == len(names) and strings[0] == "CC1C2N1CC1=C2CC=C1" and names[0] == "69719"
    res = gdb13_model(golden_dir)
    rules = VM.Rules(**GDB13_ARGS)
    rejected = [(k + 2, s, int(res["status"][k])) for k, s in enumerate(strings) if res["status"][k] & RM.RD_ERROR]
    assert rejected == []                                                   # by line of the file; the cap is zero
    assert not (res["status"] & ~RM.RD_INFO).any() and (res["n_nodes"] > 0).all() and res["n_nodes"].max() == GDB13_N
    for k, s in enumerate(strings):
        v = VM.judge(res["nodes"][k], res["edges"][k], int(res["n_nodes"][k]), rules)
        assert v["valid"] == 1 and not v["status"] & ~VM.VAL_H_MISMATCH, (k + 2, s, v["status"])
        assert SM.same(SM.graph_of(res["nodes"][k], res["edges"][k], None, rules), SM.read(s)), (k + 2, s)
    assert any("[N+]" in s for s in strings) and any("[O-]" in s for s in strings) and any("#" in s for s in strings)


# ---- 4: one string per status bit; the boundary ---------------------------------------------------------------------

def test_one_string_per_status_bit():
    cases = status_cases()
    seen = 0
    for name, (s, r, N, kw, want) in cases.items():
        got = read_string(s, rules_of(r), N, **kw)
        assert got["status"] == want, (name, s, got["status"], want)
        seen |= want
        if want & RM.RD_ERROR:
            assert not got["nodes"].any() and not got["edges"].any() and (got["atom_pos"] == -1).all(), name
            assert got["n_nodes"] == (6 if name == "too_many" else 0), name  # the need, so that the caller can ask again
        else:
            assert got["n_nodes"] > 0 and (got["atom_pos"][:got["n_nodes"]] >= 0).all(), name
    assert seen == RM.RD_ERROR | RM.RD_INFO                                 # every bit has its string
    again = read_string(cases["too_many"][0], rules_of(cases["too_many"][1]), 6)
    assert again["status"] == 0 and again["n_nodes"] == 6
    dropped = read_string("F/C=C\\F", model_rules("chem"), 4, drop_stereo=True)
    plain = read_string("FC=CF", model_rules("chem"), 4)
    assert np.array_equal(dropped["nodes"], plain["nodes"]) and np.array_equal(dropped["edges"], plain["edges"])
    one = read_string("C=1CC1", VM.Rules(**GDB13_ARGS), 4)
    other = read_string("C1CC=1", VM.Rules(**GDB13_ARGS), 4)
    both = read_string("C=1CC=1", VM.Rules(**GDB13_ARGS), 4)
    assert one["edges"][0, 2, 1] == 1 and np.array_equal(one["edges"], other["edges"]) and np.array_equal(one["edges"], both["edges"])
    # a length outside the row, and NULL against explicit lengths
    text, length = RM.pack(["CCO", "C"], 16)
    r = VM.Rules(**GDB13_ARGS)
    assert RM.read_one(text[0], 17, r, 4, 12, 3)["status"] == RM.RD_SYNTAX == RM.read_one(text[0], -1, r, 4, 12, 3)["status"]
    assert RM.read_one(text[0], 4, r, 4, 12, 3)["status"] == RM.RD_SYNTAX    # the zero byte inside an explicit length
    assert RM.read_one(text[0], None, r, 4, 12, 3)["n_nodes"] == 3 == RM.read_one(text[0], 3, r, 4, 12, 3)["n_nodes"]
    assert RM.read_one(text[0], 2, r, 4, 12, 3)["n_nodes"] == 2


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    decl = re.search(r"^int\s+gi_smiles_read\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(L.SIGNATURES["gi_smiles_read"][1]) == len(decl.split(",")) == 23 and hasattr(lib, "gi_smiles_read")
    assert hdr.index("gi_mol_smiles(") < hdr.index("gi_smiles_read(")
    bits = 0
    for name in ("MULTI_BOND", "EMPTY", "SELF_LOOP", "OVER", "FRAGMENTS", "AROMATIC", "TOO_MANY", "SYNTAX", "RING_OPEN",
                 "RING_ORDER", "ELEMENT", "CHARGE", "HCOUNT", "BOND_ORDER", "STEREO", "STEREO_DROPPED", "UNSUPPORTED"):
        value = int(re.search(rf"#define\s+GI_SMR_{name}\s+(\d+)\b", hdr).group(1))
        assert getattr(L, "SMR_" + name) == value == getattr(RM, "RD_" + name), name
        assert value in analyze.READ_STATUS_MESSAGES and bits & value == 0
        bits |= value
    assert set(analyze.READ_STATUS_MESSAGES) == {1 << k for k in range(32) if bits >> k & 1}
    assert L.SMR_ERROR == RM.RD_ERROR == bits & ~RM.RD_INFO
    assert (L.SMR_MULTI_BOND, L.SMR_EMPTY, L.SMR_SELF_LOOP, L.SMR_OVER, L.SMR_FRAGMENTS, L.SMR_AROMATIC, L.SMR_TOO_MANY) == \
        (L.MOL_MULTI_BOND, L.SMI_EMPTY, L.SMI_SELF_LOOP, L.SMI_OVER, L.SMI_FRAGMENTS, L.SMI_AROMATIC, L.SMI_TRUNCATED)
    assert analyze.describe_read_status(0) == "read" and "kekulised" in analyze.describe_read_status(L.SMR_AROMATIC)
    assert "gi_smiles_read.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_smiles_read.hip")).read()
    assert "getenv" not in src and "hipMemset" not in src and "atomicAdd(" not in src   # nothing cleared, no global atomics
    # the LDS budget at the limits: rows of N = 128, Fe = 8, the string and its classes, and the static arrays
    assert 8 * 128 * 16 + 2 * L.SMI_MAX_LEN + 12 * 1024 <= 64 * 1024
    lay = ReadMolecules.layout(3, 5, 8, 3)
    assert lay["atom_pos"] == (0, 60, "int32", (3, 5)) and lay["nodes"][0] % 16 == 0 and lay["edges"][0] == lay["nodes"][0] + 120
    assert ReadMolecules.nbytes(3, 5, 8, 3) == lay["edges"][0] + 3 * 5 * 5 * 3
    # argument checks that need no device: nothing is launched, nothing is written, for any of these
    def call(G=0, N=13, Fn=12, Fe=3, max_len=160, A=5, C=3, H=4, none=0, drop=0):
        return lib.gi_smiles_read(G, N, Fn, Fe, None, None, max_len, A, C, H, None, None, None, None, None, none, drop,
                                  None, None, None, None, None, None)
    assert call() == 0                                                     # an empty batch: no launch
    assert call(G=1) == -1                                                 # no buffers
    assert call(N=129) == -1 and call(N=0) == -1 and call(Fe=9) == -1 and call(Fe=0) == -1 and call(G=-1) == -1
    assert call(Fn=513, H=0) == -2 and call(Fn=11) == -1 and call(A=0) == -1 and call(C=0) == -1 and call(H=-1) == -1
    assert call(none=-1) == -1 and call(none=1) == 0 and call(Fn=14, none=2) == -1 and call(Fn=14, none=1) == 0
    assert call(drop=2) == -1 and call(drop=1) == 0
    assert call(max_len=0) == -1 and call(max_len=24) == -1 and call(max_len=8192) == 0 and call(max_len=8208) == -2
    assert call(N=128, Fe=8, Fn=512, H=0, max_len=8192) == 0


def test_python_boundary_raises(tmp_path):
    host_rules = analyze.ValenceRules(device=None, **GDB13_ARGS)
    with pytest.raises(TypeError, match="ValenceRules"):
        read_smiles(["C"], [5, 3], 13)
    with pytest.raises(ValueError, match="'error' or 'drop'"):
        read_smiles(["C"], host_rules, 13, stereo="keep")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_n_nodes"):
            read_smiles(["C"], host_rules, bad)
    with pytest.raises(ValueError, match="max_n_nodes <= 128"):
        read_smiles(["C"], host_rules, 129)
    with pytest.raises(ValueError, match="none_chirality"):
        read_smiles(["C"], host_rules, 13, n_chirality=3, none_chirality=3)
    with pytest.raises(ValueError, match="Fn <= 512"):
        read_smiles(["C"], host_rules, 13, n_chirality=501)
    with pytest.raises(RuntimeError, match="device=None"):
        read_smiles(["C"], host_rules, 13)
    with pytest.raises(ValueError, match="one or two ASCII letters"):
        read_smiles(["C"], analyze.ValenceRules(["C", "Xx1"], [0], allowed={("Xx1", 0): (1,)}, masses={"Xx1": 1},
                                                device=None), 13)
    with pytest.raises(ValueError, match="not ASCII"):
        pack_strings(["C", "É"], device="cpu")
    with pytest.raises(TypeError, match="str or bytes"):
        pack_strings(["C", 5], device="cpu")
    for bad in (0, 24, 8208, 16.0, True):
        with pytest.raises(ValueError, match="max_len"):
            pack_strings(["C"], max_len=bad, device="cpu")
    with pytest.raises(ValueError, match="string 1 has 17 bytes"):
        pack_strings(["C", "C" * 17], max_len=16, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU"):
        pack_strings(["C"], device="cpu")
    with pytest.raises(ValueError, match="batch"):
        read_smi(str(tmp_path / "none.smi"), host_rules, 13, batch=0)
    text, length = RM.pack(["CCO", "C"])
    assert text.shape == (2, 16) and length.tolist() == [3, 1] and RM.pack([])[0].shape == (0, 16)
    if not torch.cuda.is_available():
        return
    rules = analyze.ValenceRules(**GDB13_ARGS)                              # raised before anything is launched
    with pytest.raises(RuntimeError, match="no CPU"):
        read_smiles(torch.zeros(2, 16, dtype=torch.uint8), rules, 13)
    dev_text = torch.zeros(2, 32, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="uint8"):
        read_smiles(dev_text.to(torch.int8), rules, 13)
    with pytest.raises(ValueError, match="max_len"):
        read_smiles(dev_text[:, :24].contiguous(), rules, 13)
    with pytest.raises(ValueError, match="contiguous"):
        read_smiles(dev_text[:, :16], rules, 13)
    with pytest.raises(RuntimeError, match="length"):
        read_smiles(dev_text, rules, 13, length=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="length"):
        read_smiles(dev_text, rules, 13, length=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="length"):
        read_smiles(["C"], rules, 13, length=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="bond_orders is required"):
        read_smiles(["C"], rules, 13, n_bond_types=2)
