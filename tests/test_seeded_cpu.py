"""CPU: seeded generation's spec and boundary.  tests/seed_grow_model.py (grow_oracle's round plus the refill from a
seed bank) with a bank of the empty seed alone reproduces grow_oracle.run_oracle — and so golden_grow.npz, the
unmodified reference loop — bit for bit; the new C ABI symbols are declared, exported and bound with the ABI version
unchanged and gi_grow_seed_desc's ctypes mirror matches a compiler probe; the Python entry points refuse what needs the
device; ``likelihood.completion_hot`` (the mask behind ``given_actions``) against tests/likelihood_model.py on the
molecules of golden_likelihood.npz."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from tests import grow_oracle as GO
from tests import likelihood_model as LM
from tests import seed_grow_model as SM
from tests.test_likelihood_cpu import ORACLE_LOGITS_BAR, golden, oracle_logits, route_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("nodes", "edges", "n_nodes", "likelihoods", "generated_nodes", "generated_edges", "generated_n_nodes",
         "generated_likelihoods", "properly_terminated")
NEW_SYMBOLS = ("gi_grow_seeded_state_words", "gi_grow_seed_init", "gi_grow_graphs_seeded", "gi_grow_graphs_rl_seeded")
CONFIGS = ["atoms_charges", "imp_h_chirality", "index_error"]


def config(golden_dir, name):
    G = np.load(os.path.join(golden_dir, "golden_grow.npz"))
    p = f"{name}::cfg::"
    return {k[len(p):]: G[k].tolist() for k in G.files if k.startswith(p)}


# ---- the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", CONFIGS)
def test_empty_seed_bank_reproduces_the_unseeded_oracle_bit_for_bit(golden_dir, name, S):
    cfg = config(golden_dir, name)
    N, groups, Fe, _, _ = GO.config_dims(cfg)
    ref, ref_draw, _ = GO.run_oracle(cfg)
    s, draw = SM.run_seeded_oracle(cfg, SM.empty_bank(N, sum(groups), Fe, S))
    assert (s["n"], s["round"], s["error"]) == (ref["n"], ref["round"], ref["error"])
    for k in STATE:
        assert s[k].dtype == ref[k].dtype and np.array_equal(s[k], ref[k]), (name, k)
    assert draw.margin == ref_draw.margin
    B, n = int(cfg["B"]), s["n"]
    # provenance: every written row names a seed of the bank, the rows never written stay -1
    assert s["slot_seed"][0] == -1 and (s["gen_seed"][n:] == -1).all()
    assert ((s["gen_seed"][:n] >= 0) & (s["gen_seed"][:n] < S)).all()
    assert ((s["slot_seed"][1:] >= 0) & (s["slot_seed"][1:] < S)).all()


@pytest.mark.parametrize("S", [1, 3, 100])
@pytest.mark.parametrize("name", ["atoms_charges", "imp_h_chirality"])
def test_seeded_model_keeps_every_seed_inside_its_product(golden_dir, name, S):
    cfg = config(golden_dir, name)
    N, groups, Fe, _, _ = GO.config_dims(cfg)
    B = int(cfg["B"])
    bank = SM.mixed_bank(N, groups, Fe, S)
    if S >= 3:
        assert bank["n_nodes"][:3].tolist() == [0, 1, N]
    s, draw = SM.run_seeded_oracle(cfg, bank)
    assert s["error"] == 0 and s["n"] >= B
    assert draw.margin > 1e-4                                  # the GPU loop test draws the same actions
    n = s["n"]
    # a row's seed is one of the first fill's, (g - 1) mod S, or the refill (B - 1 + row') mod S of an earlier row
    handed_out = {(g - 1) % S for g in range(1, B)}
    for row in range(n):
        seed = int(s["gen_seed"][row])
        assert seed in handed_out, row
        handed_out.add((B - 1 + row) % S)
        ns = int(bank["n_nodes"][seed])
        assert np.array_equal(s["generated_nodes"][row, :ns], bank["nodes"][seed, :ns].astype(np.float32))
        sub = s["generated_edges"][row, :ns, :ns]
        assert (sub >= bank["edges"][seed, :ns, :ns]).all()
        extra = np.argwhere((sub != 0) & (bank["edges"][seed, :ns, :ns] == 0))
        assert all(ns - 1 in (i, j) for i, j, _ in extra)
        assert s["generated_n_nodes"][row] >= ns
    # the live slots hold their recorded seed (or a growth of it)
    for g in range(1, B):
        seed = int(s["slot_seed"][g])
        ns = int(bank["n_nodes"][seed])
        assert np.array_equal(s["nodes"][g, :ns], bank["nodes"][seed, :ns].astype(np.float32))


def test_refill_rule_is_round_robin_over_the_bank():
    """Two rounds by hand: B = 4, S = 3, every graph but 0 terminates each round."""
    N, groups, Fe, B = 3, [2, 2], 2, 4
    bank = SM.mixed_bank(N, groups, Fe, 3)
    s = SM.new_seeded_state(B, N, 4, Fe, 4, 16, bank)
    s["target"] = 100
    assert s["slot_seed"].tolist() == [-1, 0, 1, 2]
    action = np.zeros((B, 4), np.int32)
    action[1:, 0] = 2
    action[0] = [0, 0, 0, 0]
    like = np.full(B, 0.5, np.float32)
    flags = np.zeros(B, np.int32)
    SM.seeded_round(s, action, like, flags, groups, Fe, bank)
    assert s["n"] == 3 and s["gen_seed"][:4].tolist() == [0, 1, 2, -1]
    assert s["slot_seed"].tolist() == [-1, (3 + 0) % 3, (3 + 1) % 3, (3 + 2) % 3]
    SM.seeded_round(s, action, like, flags, groups, Fe, bank)
    assert s["gen_seed"][:7].tolist() == [0, 1, 2, 0, 1, 2, -1]
    assert s["slot_seed"].tolist() == [-1, 0, 1, 2]
    for g in range(1, B):
        assert np.array_equal(s["nodes"][g], bank["nodes"][s["slot_seed"][g]].astype(np.float32))
        assert s["n_nodes"][g] == bank["n_nodes"][s["slot_seed"][g]]
        assert (s["likelihoods"][g] == 0).all()
    # generated likelihood rows: the terminate alone (the completion of a seed that was finished at once)
    assert (s["generated_likelihoods"][:6, 0] == [0.5, 0.5, 0.5, 0, 0, 0]).all()
    assert (s["generated_likelihoods"][3:6, 1] == 0.5).all()


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    assert re.search(r"#define GI_ABI_VERSION 18\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in L.SIGNATURES, name
    assert "typedef struct gi_grow_seed_desc" in header
    lib = L.load()                                               # binds every symbol of SIGNATURES or raises
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.gi_abi_version() == L.ABI_VERSION == 18
    assert lib.gi_grow_seeded_state_words(1000) == L.GROW_STATE_WORDS + 3000
    assert lib.gi_grow_seeded_state_words(-1) == -1
    assert lib.gi_grow_state_words(1000) == L.GROW_STATE_WORDS + 1000          # the existing sizes stay
    assert lib.gi_grow_rl_state_words(1000) == L.GROW_STATE_WORDS + 2000
    # host-side argument checks need no device
    d, sd = L.GrowDesc(), L.GrowSeedDesc()
    assert lib.gi_grow_seed_init(None, C.byref(sd), None, None) == -1
    assert lib.gi_grow_graphs_seeded(None, C.byref(sd), None) == -1
    assert lib.gi_grow_graphs_rl_seeded(None, C.byref(sd), None) == -1
    d.B, d.N, d.Fn, d.Fe, d.L, d.C = 4, 3, 5, 2, 6, 8
    assert lib.gi_grow_seed_init(C.byref(d), C.byref(sd), None, None) == -1    # NULL tensors
    for f in ("nodes", "edges", "n_nodes", "likelihoods", "state"):
        setattr(d, f, 64)
    assert lib.gi_grow_seed_init(C.byref(d), None, None, None) == -1           # no bank
    sd.nodes, sd.edges, sd.n_nodes, sd.S = 64, 64, 64, 0
    assert lib.gi_grow_seed_init(C.byref(d), C.byref(sd), None, None) == -1    # S < 1


def test_seed_descriptor_matches_the_ctypes_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in L.GrowSeedDesc._fields_]
    assert fields == ["nodes", "edges", "n_nodes", "gen_seed", "S"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "graphinvent_amd.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(gi_grow_seed_desc));', '  printf("%zu\\n", sizeof(gi_grow_desc));',
           '  printf("%zu\\n", sizeof(gi_grow_rl_desc));']
    src += [f'  printf("%zu\\n", offsetof(gi_grow_seed_desc, {f}));' for f in fields]
    src += ['  return 0;', '}']
    cfile, exe = tmp_path / "seed.c", tmp_path / "seed"
    cfile.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:3] == [C.sizeof(L.GrowSeedDesc), C.sizeof(L.GrowDesc), C.sizeof(L.GrowRlDesc)]
    assert got[3:] == [getattr(L.GrowSeedDesc, f).offset for f in fields]


def test_seeded_entry_points_refuse_cpu_tensors_and_wrong_arguments():
    from graphinvent_amd import generator as GEN
    N, groups, Fe = 3, [3, 2], 2
    bank = SM.mixed_bank(N, groups, Fe, 3)
    nodes, edges = torch.from_numpy(bank["nodes"]), torch.from_numpy(bank["edges"])
    with pytest.raises(RuntimeError, match="CUDA"):
        GEN.SeedBank(nodes, edges, [N, *groups, Fe], [N, Fe])
    with pytest.raises(ValueError, match="reorder"):
        GEN.SeedBank(nodes, edges, [N, *groups, Fe], [N, Fe], reorder="canonical")
    B = 4
    t = dict(nodes=torch.zeros(B, N, 5), edges=torch.zeros(B, N, N, Fe), n_nodes=torch.zeros(B, dtype=torch.int8),
             likelihoods=torch.zeros(B, 6))
    state = torch.zeros(L.GROW_STATE_WORDS + 3 * B, dtype=torch.int32)
    with pytest.raises(TypeError, match="SeedBank"):
        GEN.seed_init(**t, state=state, seeds=bank)
    assert GEN.new_state.__defaults__ == (False, False)
    import inspect
    for fn in (GEN.build_graphs, GEN.build_graphs_rl, GEN.grow_step, GEN.grow_step_rl):
        p = inspect.signature(fn).parameters["seeds"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__


# ---- given_actions --------------------------------------------------------------------------------------------------

def completion_cases():
    """(given [140], expected fp64 partial sums from the golden's own rows, rows kept) for: nothing given, everything
    but the terminate given, and a per-molecule value in between."""
    G = golden()
    row_step = np.load(os.path.join(ROOT, "tests", "golden", "golden_routes.npz"))["gdb13::row_step"]
    row_mol = route_set()[3]
    lengths = np.bincount(row_mol, minlength=140)                          # n_edges + 2
    assert np.array_equal(np.bincount(row_mol, weights=row_step == 0), np.ones(140))
    rng = np.random.default_rng(11)
    between = (rng.random(140) * (lengths - 1)).astype(np.int32)
    between[:3] = [1, lengths[1] - 2, 1]
    out = {}
    for name, given in (("none", np.zeros(140, np.int32)), ("all", (lengths - 1).astype(np.int32)),
                        ("between", np.clip(between, 0, lengths - 1).astype(np.int32))):
        keep = row_step <= (lengths - 1 - given)[row_mol]
        out[name] = (given, np.bincount(row_mol, weights=G["row_ll"] * keep, minlength=140),
                     np.bincount(row_mol, weights=keep, minlength=140), keep)
    return out, row_step, lengths


@pytest.mark.parametrize("case", ["none", "all", "between"])
def test_given_actions_mask_against_the_likelihood_model(case):
    from graphinvent_amd.likelihood import completion_hot
    G = golden()
    _, _, hot, row_mol, _, _, dim_f_add, dim_f_conn = route_set()
    cases, row_step, lengths = completion_cases()
    given, want, n_kept, keep = cases[case]
    h = completion_hot(torch.from_numpy(hot), torch.from_numpy(row_mol), torch.from_numpy(row_step),
                       torch.from_numpy(lengths.astype(np.int32)), torch.from_numpy(given))
    assert h.dtype == torch.int32 and np.array_equal(h.numpy(), np.where(keep, hot, -1))
    z = oracle_logits()
    slack = ORACLE_LOGITS_BAR * float(G["logit_absmax"])
    rows = LM.row_ll(z.double(), h)
    assert (rows.numpy()[~keep] == 0).all()
    mols = LM.molecule_ll(rows, torch.from_numpy(row_mol), 140).numpy()
    assert (np.abs(mols - want) <= 2 * slack * n_kept).all()
    n_add, n_conn = LM.kind_dims(dim_f_add, dim_f_conn)
    kinds = LM.molecule_kinds(rows, h, torch.from_numpy(row_mol), 140, n_add, n_conn).numpy()
    assert np.abs(kinds.sum(1) - mols).max() <= 1e-9
    if case == "none":                                                     # the stored golden value
        assert np.array_equal(h.numpy(), hot)
        assert (np.abs(mols - G["mol_ll"]) <= 2 * slack * n_kept).all()
    if case == "all":                                                      # the terminate row alone
        assert (n_kept == 1).all() and (kinds[:, :2] == 0).all()
        assert (np.abs(mols - G["row_ll"][row_step == 0]) <= 2 * slack).all()
    if case == "between":
        assert (n_kept > 1).any() and (n_kept < lengths).any()
