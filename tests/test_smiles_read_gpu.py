"""-m gpu: SMILES strings into molecules on the device (graphinvent_amd.analyze.read_smiles / read_smi: gi_smiles_read).

Every comparison is exact — nodes, edges, n_nodes, status, atom_pos, byte for byte — against the Python specification
tests/smiles_read_model.py, which tests/test_smiles_read_cpu.py pins to an independent reader, to the writer's model as
its exact inverse, to the reference's GDB-13 strings and to one hand-made string per status bit.  NO aromatic input and
NO stereo: such strings must come back with their status bit and the all-zero molecule.  Every malformed string here is
one the kernel answers with a status word."""
import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import smiles_model as SM
from tests import smiles_read_model as RM
from tests import valence_model as VM
from tests.molio import to_dev
from tests.test_smiles_cpu import SETS, hand_cases, strings_of
from tests.test_smiles_read_cpu import (BAD, GDB13_ARGS, GDB13_N, HAND_STRINGS, gdb13_model, gdb13_strings,
                                        status_cases)
from tests.test_valence_cpu import RULE_ARGS, stored_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("nodes", "edges", "n_nodes", "status", "atom_pos")
_TYPES = ["B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I", "H", "Se", "Si"]
_CHARGES = [-1, 0, 1, 2]
#: the argument sets of the rules, for the model (VM.Rules) and the device (analyze.ValenceRules) alike
ARGS = dict(RULE_ARGS, gdb13_h=GDB13_ARGS,
            wide=dict(atom_types=_TYPES[:11], formal_charge=_CHARGES, imp_H=list(range(7)),
                      allowed={(a, q): tuple(range(1, 8)) for a in _TYPES[:11] for q in _CHARGES
                               if VM.valences_of(a, q) is None}),
            wide_fill=dict(atom_types=_TYPES, formal_charge=_CHARGES,
                           allowed={(a, q): tuple(range(1, 8)) for a in _TYPES for q in _CHARGES
                                    if VM.valences_of(a, q) is None}),
            single=dict(atom_types=["C", "N"], formal_charge=[0], bond_orders=(1,)),
            single_double=dict(atom_types=["C", "N"], formal_charge=[0], bond_orders=(1, 2)),
            eight=dict(atom_types=["C", "N"], formal_charge=[0], imp_H=[3, 2, 1, 0],
                       bond_orders=(1.5, 3, 1, 2, 1, 2, 3, 1.5)))
_RULES = {}


def rules_pair(name):
    """-> (the model's rules, the device's) of an argument set, built once."""
    if not isinstance(name, str):                                           # a VM.Rules of status_cases(): by its tables
        name = next(k for k, a in ARGS.items() if a["atom_types"] == name.atom_types and
                    a["formal_charge"] == name.formal_charge and a.get("imp_H") == name.h_values and
                    [VM.ORDER2[b] for b in a.get("bond_orders", (1, 2, 3))] == name.order2)
    if name not in _RULES:
        _RULES[name] = (VM.Rules(**ARGS[name]), analyze.ValenceRules(**ARGS[name]))
    return _RULES[name]


def assert_same(res, want, what=""):
    host = dict(zip(FIELDS, res.host()))
    for name in FIELDS:
        g, w = host[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
        view = getattr(res, name)
        assert view.is_cuda and np.array_equal(view.cpu().numpy(), w), (what, name)     # the device views are the same
    assert res.nodes.dtype == torch.int8 and res.edges.is_contiguous() and res.status.dtype == torch.int32


def check(strings, rules, N, what="", n_chirality=0, none_chirality=0, stereo="error", max_len=None, want=None):
    """The device on a list of strings against the model: with explicit lengths, without, and twice for equal bits."""
    model_rules, dev_rules = rules_pair(rules)
    Fe = len(model_rules.order2)
    text, length = RM.pack(strings, max_len)
    if want is None:
        want = RM.read_batch(text, length, model_rules, N, sum(model_rules.groups) + n_chirality, Fe, none_chirality,
                             stereo == "drop")
    kw = dict(n_chirality=n_chirality, none_chirality=none_chirality, stereo=stereo, n_bond_types=Fe)
    a = analyze.read_smiles(strings, dev_rules, N, **kw) if max_len is None else None
    dt = torch.from_numpy(text).to(DEV)
    b = analyze.read_smiles(dt, dev_rules, N, length=torch.from_numpy(length).to(DEV), **kw)
    c = analyze.read_smiles(dt, dev_rules, N, **kw)                         # length = NULL: up to the first zero byte
    d = analyze.read_smiles(dt, dev_rules, N, **kw)
    for res, tag in ((a, "list"), (b, "length"), (c, "null"), (d, "again")):
        if res is not None:
            assert_same(res, want, (what, tag))
    assert all(torch.equal(getattr(c, name), getattr(d, name)) for name in FIELDS)
    return want


# ---- device against model: the fixture strings and the reference's ---------------------------------------------------

@pytest.mark.parametrize("c", SETS)
def test_device_equals_the_model_on_the_fixture_strings(golden_dir, c):
    nodes = stored_set(golden_dir, c)[0]
    N, Fn = nodes.shape[1:]
    n_chir = Fn - sum(rules_pair(c)[0].groups)
    for ranked in (False, True):
        strings = strings_of(golden_dir, c, ranked)["strings"]              # empty ones included: SMR_EMPTY
        want = check(strings, c, N, (c, ranked), n_chirality=n_chir, none_chirality=n_chir - 1 if n_chir else 0)
        assert (want["status"][[not s for s in strings]] == L.SMR_EMPTY).all()
        assert not (want["status"][[bool(s) for s in strings]] & L.SMR_ERROR).any()


def test_device_equals_the_model_on_the_gdb13_strings(golden_dir):
    strings, _ = gdb13_strings(golden_dir)
    want = check(strings, "gdb13_h", GDB13_N, "gdb13_1K", want=gdb13_model(golden_dir))
    assert len(strings) == 979 and not (want["status"] & L.SMR_ERROR).any()


def test_every_error_string_in_one_batch():
    cases = status_cases()
    groups = {}
    for name, (s, r, N, kw, _) in cases.items():
        rname = r if isinstance(r, str) else next(k for k in ("gdb13_h", "single_double") if rules_pair(k)[0].groups ==
                                                  r.groups and rules_pair(k)[0].order2 == r.order2)
        groups.setdefault((rname, N, kw.get("drop_stereo", False)), []).append(name)
    assert len(groups) >= 4
    for (rname, N, drop), names in groups.items():
        want = check([cases[k][0] for k in names], rname, N, names, stereo="drop" if drop else "error")
        assert want["status"].tolist() == [cases[k][4] for k in names]
    want = check(list(BAD + HAND_STRINGS), "wide", 24, "bad and hand strings")
    assert (want["status"][:len(BAD)] & L.SMR_ERROR).all() and not (want["status"][len(BAD):] & L.SMR_ERROR).any()
    check([c["text"] for c in hand_cases().values()], "wide", 128, "hand cases")
    # a string with several defects gets the bits of the first stage that objects, as the model orders them
    want = check(["c1ccccc1/C=C/[13CH3]!", "[C@H](F)(Cl)[Xe]", "C(=O)(1"], "wide", 24, "several defects")
    assert want["status"][0] == L.SMR_AROMATIC | L.SMR_STEREO | L.SMR_SYNTAX | L.SMR_UNSUPPORTED


# ---- the round trip on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SETS)
def test_device_round_trip(golden_dir, c):
    nodes, edges, n, _ = stored_set(golden_dir, c)
    model_rules, rules = rules_pair(c)
    A, C, H = model_rules.groups
    N, Fn = nodes.shape[1:]
    dn, de = to_dev(nodes), to_dev(edges)
    dk = None if n is None else torch.from_numpy(n).to(DEV)
    written = analyze.smiles(dn, de, dk, rules)
    read = analyze.read_smiles(written, rules, N, n_chirality=Fn - (A + C + H), n_bond_types=edges.shape[3])
    again = analyze.smiles(read.nodes, read.edges, read.n_nodes, rules)
    strings, length, status, atom_pos = written.host()
    got_n, got_e, got_k, got_status, got_pos = read.host()
    assert torch.equal(again.text, written.text) and torch.equal(again.length, written.length)
    assert again.host()[0] == strings and sum(1 for s in strings if s) > 0
    for g, s in enumerate(strings):
        if not s:
            assert got_status[g] == L.SMR_EMPTY and got_k[g] == 0 and not got_n[g].any() and not got_e[g].any()
            continue
        k = int(got_k[g])
        perm = np.argsort(atom_pos[g][:k], kind="stable")
        assert not got_status[g] & L.SMR_ERROR and (atom_pos[g][:k] >= 0).all() and (atom_pos[g][k:] == -1).all()
        assert np.array_equal(got_n[g][:k, :A + C + H], nodes[g][perm][:, :A + C + H]) and not got_n[g][k:].any(), (c, g)
        assert np.array_equal(got_e[g][:k, :k], edges[g][perm][:, perm]) and got_e[g].sum() == edges[g].sum(), (c, g)
        assert np.array_equal(got_pos[g][:k], atom_pos[g][perm])


# ---- the edges of the kernel ---------------------------------------------------------------------------------------

def ring_fan():
    """25 atoms that open 99 ring numbers between them, a spacer, and 4 atoms that close them: 99 rings open at once."""
    text, number = "", 1
    for i in range(25):
        text += "C"
        for _ in range(4 if i < 24 else 3):
            text += SM.ring_number(number)
            number += 1
    text += "C"
    for k in range(4):
        text += "C" + "".join(SM.ring_number(4 * i + k + 1) for i in range(25) if 4 * i + k + 1 <= 99)
    return text


def edge_cases():
    """name -> (strings, rules, N, keywords of check)."""
    ladder = hand_cases()["ladder"]["text"]
    return {
        "piece_seams": (["", "C", "C" * 15, "C" * 16, "C" * 17, "C" * 32, "C" * 14 + "[NH4+]", "C" * 13 + "Cl" + "C" * 17],
                        "chem", 32, dict(max_len=32)),
        "wave_seam": (["C" * 64, "C" * 65, "C" * 61 + "[NH2+]C", "C" * 63 + "ClC", "C" * 62 + "[O-]", "[CH2]" * 128,
                       "C" * 126 + "[CH2][CH3]"], "chem", 128, {}),
        "N_128": (["C" * 128, "C" * 129, "[CH2]" * 129, "C" * 127 + "Cl", "C" * 127 + "ll"], "chem", 128, {}),
        "N_4": (["CCCC", "CCCCC", "C1CCC1", "C(C)(C)C", "C(C)(C)(C)C", "C.C.C.C", "C.C.C.C.C"], "gdb13", 4, {}),
        "N_1": (["C", "CC", "[NH4+]", ""], "gdb13", 1, {}),
        "dots": (["C(.C)C", "C.", "C1.C1", "C1.C2.C1.C2", "C1.C.C1", "C12.C1.C2", "C(.C1)C.C1", "C1.C2.C3.C1.C2.C3.C",
                  "C1.C1.C1.C1", ".C", "C(.)C"], "gdb13", 8, {}),
        "rings": ([ladder, "C1CC1C1CC1", "C1CC1.C1CC1", ring_fan(), "C%01CC1", "C0CC0", "C%99CC%99", "C%10CC%11"],
                  "wide", 32, {}),
        "ring_bond_symbols": (["C=1CC1", "C1CC=1", "C=1CC=1", "C=1CC#1", "C-1CC1", "C#1CC-1", "C=1CC-1"], "gdb13", 4, {}),
        "depth_15": (["C" + "(C" * 15 + ")" * 15, "C" + "(C" * 15 + ")" * 14, "C" + "(C" * 15 + ")" * 16], "gdb13", 16, {}),
        "depth_127": (["C" + "(C" * 127 + ")" * 127, "C" + "(=C" * 127 + ")" * 127], "gdb13", 128, {}),
        "two_letters": (["ClC", "CCl", "BrB", "CBr", "BC", "CB", "ClBr", "C(Cl)C", "Cl", "Br", "Clr", "Bl", "C[Cl]",
                         "[Br-]", "[Cl+]C"], "wide", 8, {}),
        "bracket_symbols": (["[Se]", "[Si]", "[H]", "[SeH2]", "C[Si](C)(C)C", "[H][H]", "[H+]", "[HH]", "[Sn]", "[S]", "[se]"],
                            "wide_fill", 8, {}),
        "Fe_1": (["CC", "C=C", "C#N", "C1CC1", "C-C"], "single", 4, {}),
        "Fe_8": (["CC", "C=C", "C#N", "C1=CC1", "[CH3][NH2]", "[CH4]", "[CH5]"], "eight", 4,
                 dict(n_chirality=3, none_chirality=2)),
        "G_1": (["CC(=O)O"], "gdb13", 13, {}),
        "odd_rows": (["CCO", "C[N+](=O)[O-]", "c1ccccc1"], "gdb13", 5, dict(n_chirality=1)),
        "stereo_dropped": (["F/C=C/F", "F/C=C\\F", "[C@H](F)(Cl)Br", "[C@@H](F)(Cl)Br", "[C@", "C[C@@]"], "wide", 8,
                           dict(stereo="drop")),
        "long_rows": (["C" * 100 + "(" * 20, "[" + "1" * 300, "[C" + "H" * 200 + "]", "[N-" + "9" * 400 + "]",
                       "C" + "%" * 500, "(" * 700, "[CH2+" + "1" * 50 + "]", "C" * 13 + "[" * 600], "chem", 128, {}),
    }


EDGES = edge_cases()


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_the_kernel(name):
    strings, rules, N, kw = EDGES[name]
    want = check(strings, rules, N, name, **kw)
    status, n = want["status"].tolist(), want["n_nodes"].tolist()
    if name == "piece_seams":
        assert status == [L.SMR_EMPTY, 0, 0, 0, 0, 0, 0, L.SMR_OVER] and n == [0, 1, 15, 16, 17, 32, 15, 31]
    if name == "wave_seam":
        assert status == [0, 0, 0, L.SMR_OVER, 0, 0, 0] and n == [64, 65, 63, 65, 63, 128, 128] and want["atom_pos"][2][61] == 61
    if name == "N_128":
        assert status == [0, L.SMR_TOO_MANY, L.SMR_TOO_MANY, 0, L.SMR_SYNTAX] and n == [128, 129, 129, 128, 0]
    if name == "N_4":
        assert status == [0, L.SMR_TOO_MANY, 0, 0, L.SMR_TOO_MANY, L.SMR_FRAGMENTS, L.SMR_TOO_MANY] and n == [4, 5, 4, 4, 5, 4, 5]
    if name == "N_1":
        assert status == [0, L.SMR_TOO_MANY, 0, L.SMR_EMPTY] and n == [1, 2, 1, 0]
    if name == "dots":
        F = L.SMR_FRAGMENTS
        assert status == [F, 0, 0, F, F, 0, F, F, F, L.SMR_SYNTAX, 0] and n == [3, 1, 2, 4, 3, 3, 4, 7, 4, 0, 2]
    if name == "rings":
        assert "%10" in strings[0] and "%11" in strings[0] and status[:3] == [0, 0, L.SMR_FRAGMENTS]
        assert status[3] == L.SMR_OVER and n[3] == 30 and want["edges"][3].sum() == 2 * (29 + 99)    # 99 open at once
        assert status[4:] == [0, 0, 0, L.SMR_RING_OPEN]
    if name == "ring_bond_symbols":
        assert status == [0, 0, 0, L.SMR_RING_ORDER, 0, L.SMR_RING_ORDER, L.SMR_RING_ORDER]
        assert (want["edges"][:3, 0, 2, 1] == 1).all() and want["edges"][4, 0, 2, 0] == 1
    if name == "depth_15":
        assert status == [0, L.SMR_SYNTAX, L.SMR_SYNTAX] and n[0] == 16
    if name == "depth_127":
        assert status == [0, 0] and n == [128, 128] and want["edges"][1, 5, 6, 1] == 1
    if name == "two_letters":
        assert status == [0] * 10 + [L.SMR_SYNTAX] * 2 + [0] * 3 and n[:10] == [2, 2, 2, 2, 2, 2, 2, 3, 1, 1]
    if name == "bracket_symbols":
        assert status == [0] * 8 + [L.SMR_ELEMENT, 0, L.SMR_AROMATIC] and n[:8] == [1, 1, 1, 1, 5, 2, 1, 1]
    if name == "Fe_1":
        assert status == [0, L.SMR_BOND_ORDER, L.SMR_BOND_ORDER, 0, 0] and want["edges"].shape[-1] == 1
    if name == "Fe_8":
        assert status == [0, 0, 0, 0, 0, L.SMR_HCOUNT, L.SMR_HCOUNT] and want["edges"].shape[-1] == 8
        assert want["edges"][0, 0, 1, 2] == 1 and want["edges"][1, 0, 1, 3] == 1 and want["edges"][2, 0, 1, 1] == 1
        assert want["nodes"][4, 0].tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0, 1]      # C | 0 | H 3 | chirality entry 2
    if name == "odd_rows":
        assert (5 * 9) % 16 and status == [0, 0, L.SMR_AROMATIC] and (want["nodes"][0, :3, 8] == 1).all()
    if name == "stereo_dropped":
        assert status == [L.SMR_STEREO_DROPPED] * 4 + [L.SMR_STEREO_DROPPED | L.SMR_SYNTAX, L.SMR_STEREO_DROPPED]
        assert np.array_equal(want["edges"][0], want["edges"][1]) and np.array_equal(want["nodes"][2], want["nodes"][3])
    if name == "long_rows":
        assert all(s & L.SMR_ERROR for s in status) and not want["nodes"].any()


def test_empty_batch_single_string_and_streams(golden_dir):
    _, rules = rules_pair("gdb13")
    none = analyze.read_smiles([], rules, 13)
    nodes, edges, n, status, atom_pos = none.host()
    assert nodes.shape == (0, 13, 8) and edges.shape == (0, 13, 13, 3) and n.shape == status.shape == (0,)
    assert atom_pos.shape == (0, 13) and len(none) == 0 and none.nodes.shape == (0, 13, 8)
    strings = gdb13_strings(golden_dir)[0][:300]
    want = RM.read_batch(strings, None, rules_pair("gdb13")[0], 13)
    a = analyze.read_smiles(strings, rules, 13)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = analyze.read_smiles(strings, rules, 13)
    side.synchronize()
    assert_same(a, want, "default stream")
    assert_same(b, want, "side stream")
    # the writer's own result as the argument, its TRUNCATED rows included: a length past the row is SMR_SYNTAX
    fix_n, fix_e, _, _ = stored_set(golden_dir, "gdb13")
    written = analyze.smiles(to_dev(fix_n), to_dev(fix_e), None, rules, max_len=16)
    read = analyze.read_smiles(written, rules, 13)
    w_strings, w_length, w_status, _ = written.host()
    assert (w_status & L.SMI_TRUNCATED).any() and not (w_status & L.SMI_TRUNCATED).all()
    want = RM.read_batch(written.text.cpu().numpy(), w_length, rules_pair("gdb13")[0], 13)
    assert_same(read, want, "the writer's result")
    assert ((want["status"] == L.SMR_SYNTAX) == ((w_status & L.SMI_TRUNCATED) != 0)).all()


def test_read_smi_with_a_short_last_batch(golden_dir, tmp_path):
    import os
    strings, names = gdb13_strings(golden_dir)
    _, rules = rules_pair("gdb13_h")
    want = gdb13_model(golden_dir)
    got = analyze.read_smi(os.path.join(golden_dir, "smiles_read_gdb13_1K.smi"), rules, GDB13_N, batch=256)   # 979 = 3 * 256 + 211
    assert len(got) == 979 and got.names == names
    for name in ("nodes", "edges", "n_nodes", "status"):
        t = getattr(got, name)
        assert t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), want[name]), name
    one = analyze.read_smi(os.path.join(golden_dir, "smiles_read_gdb13_1K.smi"), rules, GDB13_N)
    assert torch.equal(one.nodes, got.nodes) and torch.equal(one.edges, got.edges) and torch.equal(one.status, got.status)
    # write_smi -> read_smi: the placeholder stays in its row with its status, no header is no problem, names are optional
    path = tmp_path / "mixed.smi"
    analyze.write_smi(str(path), ["CCO", "", "C1CC1", "c1ccccc1"])
    back = analyze.read_smi(str(path), rules, GDB13_N, batch=3)
    assert back.names == ["0", "1", "2", "3"] and back.status.tolist() == [0, L.SMR_ELEMENT, 0, L.SMR_AROMATIC]
    assert back.n_nodes.tolist() == [3, 0, 3, 0] and back.nodes.shape == (4, 13, 12)
    path.write_text("CCO\n\nCC first second\n")
    bare = analyze.read_smi(str(path), rules, GDB13_N)
    assert bare.names == ["", "", "first"] and bare.status.tolist() == [0, L.SMR_EMPTY, 0] and bare.n_nodes.tolist() == [3, 0, 2]
    path.write_text("")
    assert len(analyze.read_smi(str(path), rules, GDB13_N)) == 0


def test_training_from_a_smi_file():
    from examples.train_from_smi import train
    history = train(epochs=2, batch=64, verbose=False)                      # .smi -> read_smi -> RouteLoader("bfs") -> steps
    assert len(history) == 2 and all(np.isfinite(h) and h > 0 for h in history)
