"""-m gpu: SMILES strings WITH AROMATIC INPUT into molecules on the device (analyze.read_smiles / read_smi with
aromatic="kekulize": gi_smiles_read_arom, the AROM instantiation of smiles_read_kernel).

Every comparison is exact — nodes, edges, n_nodes, status, atom_pos, byte for byte — against the Python specification
tests/kekule_read_model.py, which tests/test_kekulize_cpu.py pins to the old model, to hand-written bond lists, to the
defining properties, to the valence model and the writer's round trip on the 863 DRD2 strings and to networkx on
generated ring systems.  THE KEKULISATION IS THE LIBRARY'S OWN RULE, NOT RDKit'S.  Every malformed string here is one the
kernel answers with a status word."""
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import kekule_read_model as KM
from tests import smiles_read_model as RM
from tests import valence_model as VM
from tests.test_kekulize_cpu import (DRD2_ARGS, DRD2_N, HAND_FORCED, HAND_SEVERAL, drd2_model, drd2_strings, error_cases,
                                     generated_model, generated_strings)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("nodes", "edges", "n_nodes", "status", "atom_pos")
_RULES = {}


def rules_pair(args=DRD2_ARGS):
    """-> (the model's rules, the device's) of an argument set, built once."""
    key = repr(sorted(args.items()))
    if key not in _RULES:
        _RULES[key] = (VM.Rules(**args), analyze.ValenceRules(**args))
    return _RULES[key]


def assert_same(res, want, what=""):
    host = dict(zip(FIELDS, res.host()))
    for name in FIELDS:
        g, w = host[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check(strings, N, what="", args=DRD2_ARGS, max_len=None, want=None, lengths=True):
    """The device with aromatic="kekulize" on a list of strings against the model: the list itself, the byte tensor with
    explicit lengths and without."""
    model_rules, dev_rules = rules_pair(args)
    text, length = RM.pack(strings, max_len)
    if want is None:
        want = KM.read_batch(text, length, model_rules, N, aromatic=True)
    if max_len is None:
        assert_same(analyze.read_smiles(strings, dev_rules, N, aromatic="kekulize"), want, (what, "list"))
    if lengths:
        dt = torch.from_numpy(text).to(DEV)
        b = analyze.read_smiles(dt, dev_rules, N, length=torch.from_numpy(length).to(DEV), aromatic="kekulize")
        c = analyze.read_smiles(dt, dev_rules, N, aromatic="kekulize")      # length = NULL: up to the first zero byte
        assert_same(b, want, (what, "length"))
        assert_same(c, want, (what, "null"))
    return want


# ---- device against model on every corpus ---------------------------------------------------------------------------

def test_hand_cases_and_errors_in_one_batch():
    cases = error_cases()
    mine = [k for k, c in cases.items() if c[1] is DRD2_ARGS]
    strings = list(HAND_FORCED) + list(HAND_SEVERAL) + [cases[k][0] for k in mine] + ["c1" + "c" * 23 + "c1", "CCO", ""]
    want = check(strings, 24, "hand cases and errors")
    status = want["status"].tolist()
    first = len(HAND_FORCED) + len(HAND_SEVERAL)
    assert all(s in (0, L.SMR_KEKULIZED) for s in status[:len(HAND_FORCED)]) and status[first - 3] == L.SMR_TOO_MANY
    assert status[first:] == [cases[k][3] if k != "too_many" else L.SMR_KEKULIZED for k in mine] + \
        [L.SMR_TOO_MANY, 0, L.SMR_EMPTY]
    assert want["n_nodes"][first + len(mine)] == 25 and L.SMR_KEKULE in status and L.SMR_RING_ORDER in status
    for name in ("no_double_type", "h_count"):
        s, args, N, expected = cases[name]
        want = check([s, "CC", "c1ccccc1"], N, name, args=args)
        assert want["status"][0] == expected and not want["nodes"][0].any()


def test_generated_ring_systems():
    want, _ = generated_model()
    check(generated_strings(), 40, "generated", want=want, lengths=False)
    assert ((want["status"] & L.SMR_KEKULE) != 0).sum() == 309


def test_drd2_strings(golden_dir):
    strings, _ = drd2_strings(golden_dir)
    want, _ = drd2_model(golden_dir)
    check(strings, DRD2_N, "drd2", want=want)
    assert len(strings) == 863 and not (want["status"] & L.SMR_READ_ERROR).any()
    assert want["edges"].nbytes == 863 * 72 * 72 * 3 < 20 * 2 ** 20


def test_the_default_is_the_old_reader_and_both_entry_points_agree(golden_dir):
    strings, _ = drd2_strings(golden_dir)
    model_rules, rules = rules_pair()
    old = RM.read_batch(strings, None, model_rules, DRD2_N)
    assert_same(analyze.read_smiles(strings, rules, DRD2_N), old, "the default")
    assert_same(analyze.read_smiles(strings, rules, DRD2_N, aromatic="error"), old, "aromatic='error'")
    assert ((old["status"] & L.SMR_AROMATIC) != 0).sum() == 859 and not old["nodes"][old["status"] != 0].any()
    # gi_smiles_read and gi_smiles_read_arom(aromatic = 0): identical buffers, poisoned first
    text, length = analyze.pack_strings(strings, device=DEV)
    G, max_len = text.shape
    A, C, H = model_rules.groups
    symbols, charges = analyze._smiles_tables("test", rules)
    order2 = rules.order2(3)
    bufs = []
    for entry in ("gi_smiles_read", "gi_smiles_read_arom"):
        res = analyze.ReadMolecules.empty(DEV, G, DRD2_N, A + C + H, 3)
        res._buf.fill_(0x5a)
        out = res._ptrs()
        head = (G, DRD2_N, A + C + H, 3, text.data_ptr(), length.data_ptr(), max_len, A, C, H, rules.allowed_mask.data_ptr(),
                order2.data_ptr(), rules.h_values.data_ptr(), charges.data_ptr(), symbols.data_ptr(), 0, 0)
        tail = (out["nodes"], out["edges"], out["n_nodes"], out["status"], out["atom_pos"],
                torch.cuda.current_stream().cuda_stream)
        fn = getattr(L.load(), entry)
        L.check(fn(*head, *tail) if entry == "gi_smiles_read" else fn(*head, 0, *tail), entry)
        assert_same(res, old, entry)
        bufs.append(res)
    assert all(torch.equal(getattr(bufs[0], name), getattr(bufs[1], name)) for name in FIELDS)
    assert L.load().gi_smiles_read_arom(*head, 2, *tail) == -1              # nothing is launched


# ---- the edges of the kernel ---------------------------------------------------------------------------------------

def test_edges_of_the_kernel():
    ring128 = "c1" + "c" * 126 + "c1"
    ring127 = "c1" + "c" * 125 + "c1"
    want = check([ring128, ring127, "c" * 128, "c1" + "c" * 127 + "c1"], 128, "N_128")
    assert want["status"].tolist() == [L.SMR_KEKULIZED, L.SMR_KEKULE, L.SMR_KEKULIZED, L.SMR_TOO_MANY]
    assert want["n_nodes"].tolist() == [128, 0, 128, 129] and want["edges"][0, 0, 127, 0] == 1 and want["edges"][0, 0, 1, 1] == 1
    pyrrole = "C" * 57 + "c1ccc[nH]1"                                       # '[' 'n' at bytes 62 63, 'H' ']' at 64 65
    colon = "C" * 58 + "c1cccc:c1"                                          # ':' at byte 64
    assert pyrrole[62:66] == "[nH]" and colon[64] == ":"
    want = check([pyrrole, colon, "C" * 63 + "c1ccccc1", "C" * 62 + "[nH]1cccc1", "C" * 60 + "[se]1cccc1"], 128, "word seams")
    assert want["status"].tolist() == [L.SMR_KEKULIZED] * 4 + [L.SMR_ELEMENT] and want["atom_pos"][0][61] == 62
    want = check(["c1ccccc1", "c1ccccc1c1ccccc1", "c1ccccc1-c1ccc", "[nH]1cccc1"], 16, "max_len 16", max_len=16)
    assert want["status"].tolist() == [L.SMR_KEKULIZED, L.SMR_KEKULIZED, L.SMR_RING_OPEN, L.SMR_KEKULIZED]
    want = check(["c1ccncc1"], 6, "G 1")
    assert want["status"].tolist() == [L.SMR_KEKULIZED] and want["n_nodes"].tolist() == [6]
    # neighbouring workgroups on different paths: aromatic, Kekule, error, blossom, empty
    mixed = ["c1ccccc1", "C1=CC=CC=C1", "c1cccc1", "CCO", "c1ccc2cccc2cc1", "", "C:C", "c1ccccc1:C", "[te]", "C1CC",
             "c1cc2ccc3ccc4ccc5ccc1c1c2c3c4c51", "x", "c", "CC(=O)Oc1ccccc1C(=O)O", "c1ccc2cc3ccccc3cc2c1", "c1ccccc1.O"] * 5
    want = check(mixed, 24, "mixed")
    assert len(set(want["status"].tolist())) >= 8


def test_empty_batch_and_streams(golden_dir):
    model_rules, rules = rules_pair()
    none = analyze.read_smiles([], rules, DRD2_N, aromatic="kekulize")
    nodes, edges, n, status, atom_pos = none.host()
    assert nodes.shape == (0, 72, 14) and edges.shape == (0, 72, 72, 3) and n.shape == status.shape == (0,) and len(none) == 0
    strings = drd2_strings(golden_dir)[0][:200]
    want, _ = drd2_model(golden_dir)
    want = {k: v[:200] for k, v in want.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = analyze.read_smiles(strings, rules, DRD2_N, aromatic="kekulize")
    side.synchronize()
    assert_same(b, want, "side stream")


# ---- downstream: the round trip, the file, training -----------------------------------------------------------------

def test_device_round_trip_on_the_drd2_strings(golden_dir):
    strings, _ = drd2_strings(golden_dir)
    _, rules = rules_pair()
    read = analyze.read_smiles(strings, rules, DRD2_N, aromatic="kekulize")
    valid = analyze.validity(read.nodes, read.edges, read.n_nodes, rules)
    written = analyze.smiles(read.nodes, read.edges, read.n_nodes, rules)
    back = analyze.read_smiles(written, rules, DRD2_N, aromatic="error")   # nothing was read back up to here
    nodes, edges, n, status, _ = read.host()
    got_n, got_e, got_k, got_status, got_pos = back.host()
    texts, _, w_status, atom_pos = written.host()
    assert bool(valid.valid.to(torch.bool).all()) and not (got_status & L.SMR_ERROR).any() and np.array_equal(got_k, n)
    for g in range(len(strings)):
        k = int(n[g])
        perm = np.argsort(atom_pos[g][:k], kind="stable")
        assert texts[g] and not any(ch in texts[g].replace("Cl", "").replace("Br", "") for ch in "bcnops:"), (g, texts[g])
        assert np.array_equal(got_n[g][:k], nodes[g][perm]) and not got_n[g][k:].any(), (g, strings[g], texts[g])
        assert np.array_equal(got_e[g][:k, :k], edges[g][perm][:, perm]) and got_e[g].sum() == edges[g].sum(), (g, strings[g])
        assert np.array_equal(got_pos[g][:k], atom_pos[g][perm])


def test_read_smi_passes_the_option_through(golden_dir):
    strings, names = drd2_strings(golden_dir)
    _, rules = rules_pair()
    want, _ = drd2_model(golden_dir)
    path = os.path.join(golden_dir, "drd2_test.smi")
    for batch in (500, 200):                                                # one short batch; two full ones and 32
        got = analyze.read_smi(path, rules, DRD2_N, aromatic="kekulize", batch=batch)
        assert len(got) == 432 and got.names == names[:432] and got.nodes.shape == (432, 72, 14)
        for name in ("nodes", "edges", "n_nodes", "status"):
            t = getattr(got, name)
            assert t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), want[name][:432]), (batch, name)
    plain = analyze.read_smi(path, rules, DRD2_N)
    assert int(((plain.status & L.SMR_AROMATIC) != 0).sum()) == 430 and not bool(plain.nodes[plain.status != 0].any())


def test_training_from_an_aromatic_smi_file(golden_dir, tmp_path):
    from examples.train_from_smi import train
    strings, names = drd2_strings(golden_dir)
    path = tmp_path / "aromatic.smi"
    path.write_text("SMILES Name\n" + "".join(f"{s} {k}\n" for s, k in zip(strings[:24], names[:24])))
    history = train(str(path), epochs=3, batch=64, verbose=False, aromatic="kekulize", **{
        "atom_types": DRD2_ARGS["atom_types"], "formal_charge": DRD2_ARGS["formal_charge"], "max_n_nodes": DRD2_N})
    assert len(history) == 3 and all(np.isfinite(h) and h > 0 for h in history) and history[-1] < history[0], history


def test_the_example_reads_the_fixture_and_writes_kekule_strings(tmp_path):
    from examples.read_aromatic_smi import run
    out = tmp_path / "kekule.smi"
    assert run(out=str(out), verbose=False) == (432, 432, 430, 432, 0)
    lines = out.read_text().splitlines()
    assert lines[0] == "SMILES Name" and len(lines) == 433 and lines[1].startswith("CC(=O)NCC1=CC=C2C(=C1)") and \
        not any(ch in "".join(lines[1:]).replace("Cl", "").replace("Br", "") for ch in "bcnops:")
