"""CPU: the specification of the SMILES reader with aromatic input (tests/kekule_read_model.py; the device side is
``analyze.read_smiles(..., aromatic="kekulize")`` / ``gi_smiles_read_arom``), and the binding and Python boundary of
the option.  No device compute is issued.

THE KEKULISATION IS THE LIBRARY'S OWN RULE, NOT RDKit'S.  The model is pinned six ways: (1) to the old model on every
string without aromatic input; (2) to hand-written bond lists where the Kekule structure is forced; (3) to the defining
properties where several structures exist; (4) to one string per error; (5) to the 863 DRD2 strings of the reference's
fine-tuning data (properties, electron parity, the valence model, the writer's round trip); (6) to networkx on generated
ring systems with odd cycles, where the matching needs augmenting paths and blossoms."""
import os
import random
import re

import networkx as nx
import numpy as np
import pytest

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import kekule_read_model as KM
from tests import smiles_model as SM
from tests import smiles_read_model as RM
from tests import valence_model as VM
from tests.test_smiles_read_cpu import BAD, GDB13_ARGS, GDB13_N, HAND_STRINGS, gdb13_model, gdb13_strings, wide_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: the DRD2 sets' preprocessing parameters: atom types, charges, implicit hydrogens
DRD2_ARGS = dict(atom_types=["C", "N", "O", "F", "S", "Cl", "Br"], formal_charge=[-1, 0, 1], imp_H=[0, 1, 2, 3])
DRD2_N = 72
Z = dict(C=6, N=7, O=8, F=9, S=16, Cl=17, Br=35)
_CACHE = {}

#: string -> (every bond "a-b" / "a=b" / "a#b" whose order is FORCED, the other (aromatic-marked) bonds "a:b" whose
#: order is one of several Kekule structures' — each of their atoms gets exactly one "=")
HAND_FORCED = {
    "c1cc[nH]c1": ("0-1 1=2 2-3 3-4 0=4", ""),
    "c1ccoc1": ("0-1 1=2 2-3 3-4 0=4", ""),
    "c1ccsc1": ("0-1 1=2 2-3 3-4 0=4", ""),
    "c1c[nH]cn1": ("0=1 1-2 2-3 3=4 0-4", ""),
    "O=c1cccc[nH]1": ("0=1 1-2 2=3 3-4 4=5 5-6 1-6", ""),
    "O=c1oc2ccccc2n1C": ("0=1 1-2 2-3 8-9 1-9 9-10", "3:4 4:5 5:6 6:7 7:8 3:8"),
    "c1ccc2[nH]ccc2c1": ("3-4 4-5 5=6 6-7", "0:1 1:2 2:3 3:7 7:8 0:8"),
    "c1cc[n+](C)cc1": ("3-4", "0:1 1:2 2:3 3:5 5:6 0:6"),
    "[O-][n+]1ccccc1": ("0-1", "1:2 2:3 3:4 4:5 5:6 1:6"),
    "c1ccccc1-c1ccccc1": ("5-6", "0:1 1:2 2:3 3:4 4:5 0:5 6:7 7:8 8:9 9:10 10:11 6:11"),
    "c1ccccc1c1ccccc1": ("5-6", "0:1 1:2 2:3 3:4 4:5 0:5 6:7 7:8 8:9 9:10 10:11 6:11"),       # biphenyl: a single linker
    "c1cccc1c1cccc1": ("0=1 1-2 2=3 3-4 0-4 4=5 5-6 6=7 7-8 8=9 5-9", ""),                      # fulvalene
    "C1=CC=CC=C1": ("0=1 1-2 2=3 3-4 4=5 0-5", ""),
    "c1ccccc1": ("", "0:1 1:2 2:3 3:4 4:5 0:5"),
    "c:1:c:c:c:c:c1": ("", "0:1 1:2 2:3 3:4 4:5 0:5"),
}
#: several Kekule structures: naphthalene, azulene, line 4 of the reference's DRD2 train.smi (a 7-ring), pyrene,
#: corannulene
HAND_SEVERAL = ("c1ccc2ccccc2c1", "c1ccc2cccc2cc1", "COc1ccccc1N1CCN(Cc2cc(C#N)c3cccccc2-3)CC1",
                "c1cc2ccc3cccc4ccc(c1)c2c34", "c1cc2ccc3ccc4ccc5ccc1c1c2c3c4c51")


def drd2_rules():
    if "rules" not in _CACHE:
        _CACHE["rules"] = VM.Rules(**DRD2_ARGS)
    return _CACHE["rules"]


def drd2_strings(golden_dir):
    """-> (the 863 strings of drd2_test.smi + drd2_valid.smi, their names)."""
    if "drd2" not in _CACHE:
        rows = []
        for name in ("drd2_test.smi", "drd2_valid.smi"):
            header, part = SM.read_smi(os.path.join(golden_dir, name))
            rows += ([tuple(header.split())] if header and header.split()[0] != "SMILES" else []) + list(part)
        _CACHE["drd2"] = [r[0] for r in rows], [r[1] for r in rows]
    return _CACHE["drd2"]


def drd2_model(golden_dir):
    """The model's result on the DRD2 strings and its traces, computed once and shared (read only)."""
    if "drd2_model" not in _CACHE:
        traces = []
        out = KM.read_batch(drd2_strings(golden_dir)[0], None, drd2_rules(), DRD2_N, aromatic=True, traces=traces)
        _CACHE["drd2_model"] = out, traces
    return _CACHE["drd2_model"]


def make(rng, W=40):
    """The generator of the ring systems: one ring of 5 .. 40 atoms, mostly c, with up to 4 chords between c atoms."""
    n = rng.randint(5, 40)
    kinds = [rng.choice(["c"] * W + ["[nH]", "o", "s"]) for _ in range(n)]
    cs = [i for i in range(n) if kinds[i] == "c"]
    chords, used = [], set()
    for _ in range(rng.randint(0, 4)):
        if len(cs) < 2:
            break
        a, b = rng.sample(cs, 2)
        if a in used or b in used or abs(a - b) in (0, 1, n - 1):
            continue
        used |= {a, b}
        chords.append((min(a, b), max(a, b)))
    dig = {i: [] for i in range(n)}
    dig[0].append(1)
    dig[n - 1].append(1)
    for k, (a, b) in enumerate(chords):
        dig[a].append(k + 2)
        dig[b].append(k + 2)
    return "".join(kinds[i] + "".join(map(str, dig[i])) for i in range(n))


def generated_strings():
    if "generated" not in _CACHE:
        rng = random.Random(20261020)
        _CACHE["generated"] = [make(rng) for _ in range(512)]
    return _CACHE["generated"]


def generated_model():
    if "generated_model" not in _CACHE:
        traces = []
        out = KM.read_batch(generated_strings(), None, drd2_rules(), 40, aromatic=True, traces=traces)
        _CACHE["generated_model"] = out, traces
    return _CACHE["generated_model"]


def error_cases():
    """name -> (string, Rules arguments, N, the status expected)."""
    single = dict(atom_types=["C", "N"], formal_charge=[0], bond_orders=(1,))
    no_h1 = dict(atom_types=["C", "N"], formal_charge=[0], imp_H=[0, 2, 3])
    return {
        "lone_c": ("c", DRD2_ARGS, 13, KM.RD_KEKULE),
        "odd_ring": ("c1cccc1", DRD2_ARGS, 13, KM.RD_KEKULE),
        "colon_between_aliphatic": ("C:C", DRD2_ARGS, 13, KM.RD_UNSUPPORTED),
        "colon_to_aliphatic": ("c1ccccc1:C", DRD2_ARGS, 13, KM.RD_UNSUPPORTED),
        "unknown_bracket_symbol": ("[te]1cccc1", DRD2_ARGS, 13, KM.RD_SYNTAX),
        "unknown_small_letter": ("x", DRD2_ARGS, 13, KM.RD_SYNTAX),
        "ring_symbols_differ": ("c:1ccccc-1", DRD2_ARGS, 13, KM.RD_RING_ORDER),
        "too_many": ("c1ccccccccccccc1", DRD2_ARGS, 13, KM.RD_TOO_MANY),
        "no_double_type": ("c1ccccc1", single, 13, KM.RD_BOND_ORDER),
        "h_count": ("[nH]1cccc1", no_h1, 13, KM.RD_HCOUNT),
    }


def read_string(s, rules, N, aromatic=True, trace=None):
    text, length = RM.pack([s])
    return KM.read_one(text[0], int(length[0]), rules, N, sum(rules.groups), len(rules.order2), aromatic=aromatic,
                       trace=trace)


def bonds_of(res, rules):
    """-> {(a, b): order} with a < b of a read molecule."""
    e = res["edges"]
    return {(int(a), int(b)): rules.order2[int(np.argmax(e[a, b]))] // 2 for a, b in np.argwhere(e.any(axis=2)) if a < b}


def parse_bonds(text):
    out = {}
    for tok in text.split():
        a, sym, b = re.fullmatch(r"(\d+)([-=#:])(\d+)", tok).groups()
        out[(min(int(a), int(b)), max(int(a), int(b)))] = {"-": 1, "=": 2, "#": 3, ":": 0}[sym]
    return out


def check_properties(res, trace, rules, what):
    """The defining properties of a read string from the model's intermediate results -> the matched pairs."""
    got = bonds_of(res, rules)
    marked = {(a, b) for (a, b) in trace["marked"] if a < b}
    need, mate = trace.get("need", [False] * trace["n"]), trace.get("mate", [-1] * trace["n"])
    assert set(got) == marked | {(a, b) for (a, b) in trace["written"] if a < b}, what
    for (a, b), o in trace["written"].items():
        if a < b:
            assert got[(a, b)] == o, (what, a, b)                           # a bond with a symbol has its written order
    doubles = {p for p in marked if got[p] == 2}
    for i in range(trace["n"]):
        mine = [p for p in doubles if i in p]
        assert len(mine) == (1 if need[i] else 0), (what, i, mine)          # exactly one, on an aromatic-marked bond
        assert (mate[i] >= 0) == bool(need[i]), (what, i)
    assert all(got[p] in (1, 2) for p in marked) and all(mate[a] == b for a, b in doubles), what
    return len(doubles)


def candidate_graph(trace):
    g = nx.Graph()
    g.add_nodes_from(i for i in range(trace["n"]) if trace["need"][i])
    g.add_edges_from((a, b) for a in range(trace["n"]) for b in trace["cand"][a] if a < b)
    return g


# ---- 1: nothing changes without aromatic input ---------------------------------------------------------------------

def test_equal_to_the_old_model_without_aromatic_input(golden_dir):
    strings, _ = gdb13_strings(golden_dir)
    rules = VM.Rules(**GDB13_ARGS)
    old = gdb13_model(golden_dir)
    assert len(strings) == 979 and not any(re.search(r"[a-z:]", s.replace("Cl", "").replace("Br", "")) for s in strings)
    for aromatic in (True, False):
        new = KM.read_batch(strings, None, rules, GDB13_N, aromatic=aromatic)
        for name in old:
            assert new[name].dtype == old[name].dtype and np.array_equal(new[name], old[name]), (aromatic, name)
    hand = list(HAND_STRINGS + BAD)
    old = RM.read_batch(hand, None, wide_rules(), 24)
    plain = [k for k, s in enumerate(hand) if not re.search(r"[bcnops:]", s)]
    assert len(plain) == len(hand) - 1 and "c1ccccc1" in hand                # the one aromatic string of BAD
    new = KM.read_batch(hand, None, wide_rules(), 24, aromatic=True)
    for name in old:
        assert np.array_equal(new[name][plain], old[name][plain]), name
    new = KM.read_batch(hand, None, wide_rules(), 24, aromatic=False)
    for name in old:
        assert np.array_equal(new[name], old[name]), name
    assert (KM.RD_KEKULE | KM.RD_KEKULIZED) & (RM.RD_ERROR | RM.RD_INFO) == 0
    assert KM.RD_ERROR == RM.RD_ERROR | KM.RD_KEKULE and KM.RD_INFO == RM.RD_INFO | KM.RD_KEKULIZED


# ---- 2, 3: hand cases -----------------------------------------------------------------------------------------------

def test_hand_cases_with_a_forced_structure():
    rules = drd2_rules()
    for s, (forced, free) in HAND_FORCED.items():
        trace = {}
        res = read_string(s, rules, 24, trace=trace)
        aromatic = bool(re.search(r"[a-z]", s))
        assert res["status"] == (KM.RD_KEKULIZED if aromatic else 0), (s, res["status"])
        got, forced, free = bonds_of(res, rules), parse_bonds(forced), parse_bonds(free)
        assert set(got) == set(forced) | set(free), (s, sorted(got))
        assert all(got[p] == o for p, o in forced.items()), (s, got)
        ring_atoms = {i for p in free for i in p}
        for i in ring_atoms:                                                # the benzene-type choice: one '=' per atom
            assert sum(1 for p in free if i in p and got[p] == 2) == 1, (s, i, got)
        check_properties(res, trace, rules, s)
    same = [read_string(s, rules, 24) for s in ("c1ccccc1-c1ccccc1", "c1ccccc1c1ccccc1")]
    assert np.array_equal(same[0]["nodes"], same[1]["nodes"]) and np.array_equal(same[0]["edges"], same[1]["edges"])
    benzene = [read_string(s, rules, 24) for s in ("C1=CC=CC=C1", "c1ccccc1", "c:1:c:c:c:c:c1")]
    for other in benzene[1:]:                                               # the same molecule: here the same choice too
        assert np.array_equal(other["nodes"], benzene[0]["nodes"]) and np.array_equal(other["edges"], benzene[0]["edges"])
    fulvalene = bonds_of(read_string("c1cccc1c1cccc1", rules, 24), rules)
    assert fulvalene[(4, 5)] == 2 and bonds_of(same[1], rules)[(5, 6)] == 1
    pyridone = read_string("O=c1cccc[nH]1", rules, 24)
    A, C = len(rules.atom_types), len(rules.formal_charge)
    assert pyridone["nodes"][:7, A + C:].argmax(axis=1).tolist() == [0, 0, 1, 1, 1, 1, 1]   # the hydrogens, after the assignment


def test_hand_cases_with_several_structures():
    rules = drd2_rules()
    counters = {}
    for s in HAND_SEVERAL:
        trace = {}
        res = read_string(s, rules, 40, trace=trace)
        assert res["status"] == KM.RD_KEKULIZED, (s, res["status"])
        pairs = check_properties(res, trace, rules, s)
        assert 2 * pairs == sum(trace["need"]) == 2 * len(nx.max_weight_matching(candidate_graph(trace), maxcardinality=True))
        v = VM.judge(res["nodes"], res["edges"], int(res["n_nodes"]), rules)
        assert v["valid"] == 1, (s, v["status"])
        for key, value in trace["counters"].items():
            counters[key] = counters.get(key, 0) + value
    _CACHE["several_counters"] = counters
    assert read_string("c1ccc2cccc2cc1", rules, 40)["n_nodes"] == 10 and read_string(HAND_SEVERAL[3], rules, 40)["n_nodes"] == 16


# ---- 4: errors ------------------------------------------------------------------------------------------------------

def test_errors_each_alone_and_in_one_batch():
    cases = error_cases()
    for name, (s, args, N, want) in cases.items():
        res = read_string(s, VM.Rules(**args), N)
        assert res["status"] == want, (name, res["status"], want)
        assert not res["nodes"].any() and not res["edges"].any() and (res["atom_pos"] == -1).all(), name
        assert res["n_nodes"] == (14 if name == "too_many" else 0), name
    names = [k for k, c in cases.items() if c[1] is DRD2_ARGS]
    batch = KM.read_batch([cases[k][0] for k in names] + ["c1ccccc1"], None, drd2_rules(), 13, aromatic=True)
    assert batch["status"].tolist() == [cases[k][3] for k in names] + [KM.RD_KEKULIZED] and len(names) == 8
    assert not batch["nodes"][:-1].any() and not batch["edges"][:-1].any() and batch["nodes"][-1].any()
    # without the option every one of them is what it was: RD_AROMATIC (with whatever else stage A and B find)
    for name in names:
        old = read_string(cases[name][0], drd2_rules(), 13, aromatic=False)
        assert old["status"] & RM.RD_ERROR and not old["status"] & (KM.RD_KEKULE | KM.RD_KEKULIZED), name
        assert old["status"] & RM.RD_AROMATIC or name in ("colon_between_aliphatic", "unknown_small_letter") or \
            old["status"] & RM.RD_TOO_MANY, name
    assert read_string("C:C", drd2_rules(), 13, aromatic=False)["status"] == RM.RD_AROMATIC


# ---- 5: the DRD2 strings --------------------------------------------------------------------------------------------

def test_drd2_strings_read_and_are_chemistry(golden_dir):
    strings, names = drd2_strings(golden_dir)
    rules = drd2_rules()
    out, traces = drd2_model(golden_dir)
    A, C, H = rules.groups
    assert len(strings) == 863 == len(names) and max(len(s) for s in strings) < 160
    assert not (out["status"] & KM.RD_ERROR).any() and out["n_nodes"].max() == 68
    lower = np.array([bool(re.search(r"[bcnops]", s.replace("Cl", "").replace("Br", ""))) for s in strings])
    assert lower.sum() == 859 and np.array_equal((out["status"] & KM.RD_KEKULIZED) != 0, lower)
    assert not (out["status"] & ~(KM.RD_KEKULIZED | RM.RD_INFO)).any()
    invalid, odd = [], []
    for g, s in enumerate(strings):
        n = int(out["n_nodes"][g])
        res = {k: out[k][g] for k in out}
        pairs = check_properties(res, traces[g], rules, (g, s))
        if lower[g]:
            assert pairs == len(nx.max_weight_matching(candidate_graph(traces[g]), maxcardinality=True)), (g, s)
        nodes = out["nodes"][g][:n]
        electrons = sum(Z[rules.atom_types[a]] for a in nodes[:, :A].argmax(axis=1)) + \
            sum(rules.h_values[h] for h in nodes[:, A + C:].argmax(axis=1)) - \
            sum(rules.formal_charge[c] for c in nodes[:, A:A + C].argmax(axis=1))
        if electrons % 2:
            odd.append(g)
        v = VM.judge(out["nodes"][g], out["edges"][g], n, rules)
        if v["valid"] != 1 or v["status"] & ~VM.VAL_H_MISMATCH:
            invalid.append(g)
        # the writer gives it a string, and the reader without the option reads that string back as the same molecule
        written = SM.write(out["nodes"][g], out["edges"][g], n, rules)
        text = written["text"].decode()
        assert text and not re.search(r"[a-z:]", text.replace("Cl", "").replace("Br", "")), (g, s, text)
        back = read_string(text, rules, DRD2_N, aromatic=False)
        perm = np.argsort(written["atom_pos"][:n], kind="stable")
        assert back["status"] & ~RM.RD_INFO == 0 and back["n_nodes"] == n, (g, s, text, back["status"])
        assert np.array_equal(back["nodes"][:n], out["nodes"][g][perm]), (g, s, text)
        assert np.array_equal(back["edges"][:n, :n], out["edges"][g][perm][:, perm]), (g, s, text)
    assert odd == [] and invalid == []


# ---- 6: matching in general graphs ----------------------------------------------------------------------------------

def test_matching_against_networkx_on_generated_ring_systems():
    strings = generated_strings()
    rules = drd2_rules()
    out, traces = generated_model()
    assert len(strings) == 512 and len(set(strings)) > 400
    classes = dict(none=0, greedy=0, augmented=0)
    counters = dict(_CACHE.get("several_counters") or {})
    for g, s in enumerate(strings):
        trace = traces[g]
        assert not out["status"][g] & (KM.RD_ERROR & ~KM.RD_KEKULE), (g, s, out["status"][g])
        best = nx.max_weight_matching(candidate_graph(trace), maxcardinality=True)
        perfect = 2 * len(best) == sum(trace["need"])
        assert bool(out["status"][g] & KM.RD_KEKULE) == (not perfect), (g, s)
        for key, value in trace["counters"].items():
            counters[key] = counters.get(key, 0) + value
        if not perfect:
            classes["none"] += 1
            assert out["n_nodes"][g] == 0 and not out["edges"][g].any()
            continue
        classes["augmented" if trace["counters"]["searches"] else "greedy"] += 1
        assert check_properties({k: out[k][g] for k in out}, trace, rules, (g, s)) == len(best)
    print("classes", classes, "counters", counters)
    assert all(v >= 0.10 * 512 for v in classes.values()), classes          # each class is there to be tested
    if "several_counters" not in _CACHE:
        for s in HAND_SEVERAL:
            trace = {}
            read_string(s, rules, 40, trace=trace)
            for key, value in trace["counters"].items():
                counters[key] = counters.get(key, 0) + value
    assert counters["augmentations"] > 0 and counters["blossoms"] > 0, counters


# ---- the binding and the Python boundary ----------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    decl = re.search(r"^int\s+gi_smiles_read_arom\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    old = re.search(r"^int\s+gi_smiles_read\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(L.SIGNATURES["gi_smiles_read_arom"][1]) == len(decl.split(",")) == 24 and hasattr(lib, "gi_smiles_read_arom")
    assert [a.split()[-1] for a in decl.split(",")] == [a.split()[-1] for a in old.split(",")][:17] + ["aromatic"] + \
        [a.split()[-1] for a in old.split(",")][17:]
    for name, bit in (("KEKULE", 67108864), ("KEKULIZED", 134217728)):
        assert int(re.search(rf"#define\s+GI_SMR_{name}\s+(\d+)\b", hdr).group(1)) == bit == getattr(L, "SMR_" + name) == \
            getattr(KM, "RD_" + name)
        assert bit in analyze.KEKULE_STATUS_MESSAGES and bit not in analyze.READ_STATUS_MESSAGES
    assert "GI_SMR_UNSUPPORTED | GI_SMR_KEKULE)" in hdr and L.SMR_READ_ERROR == KM.RD_ERROR == L.SMR_ERROR | L.SMR_KEKULE
    assert "Kekule structure" in analyze.describe_read_status(L.SMR_KEKULE)
    assert "kekulised" in analyze.describe_read_status(L.SMR_KEKULIZED) and analyze.describe_read_status(0) == "read"
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_smiles_read.hip")).read()
    assert "smiles_read_kernel<true>" in src and "smiles_read_kernel<false>" in src and "atomicAdd(" not in src
    assert 8 * 128 * 16 + 2 * L.SMI_MAX_LEN + 14 * 1024 <= 64 * 1024       # the LDS budget with the matching's 2.7 KB

    def call(G=0, aromatic=1, N=13, Fn=12, Fe=3, max_len=160):
        return lib.gi_smiles_read_arom(G, N, Fn, Fe, None, None, max_len, 5, 3, 4, None, None, None, None, None, 0, 0,
                                       aromatic, None, None, None, None, None, None)
    assert call() == 0 and call(aromatic=0) == 0                            # an empty batch: no launch
    assert call(aromatic=2) == -1 and call(aromatic=-1) == -1 and call(G=1) == -1 and call(G=1, aromatic=0) == -1
    assert call(N=129) == -1 and call(Fe=9) == -1 and call(max_len=24) == -1 and call(max_len=8208) == -2


def test_python_boundary_raises():
    host_rules = analyze.ValenceRules(device=None, **GDB13_ARGS)
    for bad in ("kekulise", "drop", None, True, 1):
        with pytest.raises(ValueError, match="'error' or 'kekulize'"):
            analyze.read_smiles(["c1ccccc1"], host_rules, 13, aromatic=bad)
    with pytest.raises(RuntimeError, match="device=None"):                  # the option is checked, then the usual checks
        analyze.read_smiles(["c1ccccc1"], host_rules, 13, aromatic="kekulize")
    with pytest.raises(ValueError, match="'error' or 'kekulize'"):
        analyze.read_smi(os.path.join(ROOT, "tests", "golden", "drd2_test.smi"), host_rules, 13, aromatic="yes")
