"""CPU: the growth step's spec and boundary.  tests/grow_oracle.py (the per-round restatement of gi_grow_graphs in
action / flags form, driven by oracle/sampler_oracle.py) reproduces golden_grow.npz — made by the UNMODIFIED reference
GraphGenerator.build_graphs — bit for bit; the Python wrapper refuses what the kernel cannot take; the header, the
ctypes mirror and lib.SIGNATURES agree."""
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
from tests.golden import ref_callers as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("nodes", "edges", "n_nodes", "likelihoods", "generated_nodes", "generated_edges", "generated_n_nodes",
         "generated_likelihoods", "properly_terminated")


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "golden_grow.npz"))


def config(G, name):
    p = f"{name}::cfg::"
    return {k[len(p):]: G[k].tolist() for k in G.files if k.startswith(p)}


def check_run(G, name, s, draw, raised):
    if int(G[f"{name}::raised_round"]) >= 0:
        assert raised == int(G[f"{name}::raised_round"]), (name, raised)
        return
    assert raised < 0
    assert (s["n"], s["round"]) == (int(G[f"{name}::n_generated"]), int(G[f"{name}::rounds"]))
    for k in STATE:
        want = G[f"{name}::{k}"]
        got = s[k] if want.dtype == s[k].dtype else s[k].astype(want.dtype)
        assert np.array_equal(got, want), (name, k)
        if want.dtype == np.int8 and s[k].dtype == np.float32:
            assert np.array_equal(s[k], want.astype(np.float32)), (name, k)     # 0 / 1 features survive the cast
    assert draw.margin == float(G[f"{name}::margin"]) and draw.margin > 1e-4


@pytest.mark.parametrize("name", ["atoms_charges", "imp_h_chirality", "index_error"])
def test_restated_round_reproduces_the_unmodified_loop(golden_dir, name):
    G = golden(golden_dir)
    s, draw, cover = GO.run_oracle(config(G, name))
    raised = s["round"] if s["error"] else -1
    if s["error"]:
        assert s["error"] == GO.ERR_ROUND                         # IndexError, as the reference
    check_run(G, name, s, draw, raised)
    if name == "atoms_charges":
        assert all(v > 0 for v in cover.values()), cover
        assert (s["edges"][0, 0, 1] != 0).sum() > 1               # several bond types on graph 0's (0, 1) pair


@pytest.mark.skipif(not RC.have_reference(), reason="no reference checkout")
@pytest.mark.parametrize("name", ["atoms_charges", "imp_h_chirality", "index_error"])
def test_unmodified_reference_loop_reproduces_the_golden(golden_dir, name):
    from tests.golden import make_golden_grow as M
    G = golden(golden_dir)
    cfg = config(G, name)
    with RC.isolated():
        _, GG = RC.load("reference", M.constants(cfg))
        gen, n, raised, draw = M.run_reference(GG, cfg)
    s = {k: getattr(gen, k).numpy() for k in STATE}
    s.update(n=n, round=draw.round)
    check_run(G, name, s, draw, raised)


def _tensors(B=4, N=3, Fn=5, Fe=2, L=6, C=8, device="cpu", **over):
    t = dict(nodes=torch.zeros(B, N, Fn), edges=torch.zeros(B, N, N, Fe), n_nodes=torch.zeros(B, dtype=torch.int8),
             likelihoods=torch.zeros(B, L), generated_nodes=torch.zeros(C, N, Fn),
             generated_edges=torch.zeros(C, N, N, Fe), generated_n_nodes=torch.zeros(C, dtype=torch.int8),
             generated_likelihoods=torch.zeros(C, L), properly_terminated=torch.zeros(C, dtype=torch.int8))
    t.update(over)
    raw = dict(action=torch.zeros(B, 4, dtype=torch.int32), likelihood=torch.zeros(B),
               flags=torch.zeros(B, dtype=torch.int32))
    return t, raw


def _call(t, raw, dim_f_add=(3, 3, 2, 2), dim_f_conn=(3, 2)):
    from graphinvent_amd.generator import grow_step
    B = t["nodes"].shape[0]
    state = torch.zeros(L.GROW_STATE_WORDS + B, dtype=torch.int32)
    grow_step(**t, **raw, dim_f_add=dim_f_add, dim_f_conn=dim_f_conn, state=state)


def test_grow_step_refuses_cpu_tensors():
    t, raw = _tensors()
    with pytest.raises(RuntimeError, match="CUDA"):
        _call(t, raw)


@pytest.mark.parametrize("name,bad,exc", [
    ("n_nodes", torch.zeros(4, dtype=torch.int32), TypeError),
    ("edges", torch.zeros(4, 3, 3, 2, dtype=torch.float64), TypeError),
    ("properly_terminated", torch.zeros(8, dtype=torch.bool), TypeError),
    ("likelihoods", torch.zeros(6, 4).t(), ValueError),                       # not contiguous
    ("generated_edges", torch.zeros(8, 3, 3, 3), ValueError),                 # Fe mismatch
    ("generated_likelihoods", torch.zeros(8, 5), ValueError),                 # L mismatch
    ("properly_terminated", torch.zeros(7, dtype=torch.int8), ValueError),    # C mismatch
    ("n_nodes", torch.zeros(5, dtype=torch.int8), ValueError),
])
def test_grow_step_refuses_wrong_dtypes_and_shapes(name, bad, exc):
    t, raw = _tensors(**{name: bad})
    with pytest.raises(exc):
        _call(t, raw)


@pytest.mark.parametrize("dim_f_add,dim_f_conn", [((3, 3, 3, 2), (3, 2)),      # groups do not tile Fn = 5
                                                   ((3, 3, 2, 3), (3, 2)),      # bond type != Fe
                                                   ((4, 3, 2, 2), (4, 2)),      # N
                                                   ((3, 3, 2, 2), (3, 3))])     # Fe
def test_grow_step_checks_the_add_layout_against_the_tensors(dim_f_add, dim_f_conn):
    t, raw = _tensors()
    with pytest.raises(ValueError):
        _call(t, raw, dim_f_add, dim_f_conn)


def test_build_graphs_refuses_a_cpu_generator():
    from graphinvent_amd.generator import build_graphs
    t, _ = _tensors()

    class Gen:
        model, batch_size = None, 4
    gen = Gen()
    for k, v in t.items():
        setattr(gen, k, v)
    with pytest.raises(RuntimeError, match="CUDA"):
        build_graphs(gen, (3, 3, 2, 2), (3, 2))


def test_header_declares_the_growth_step_and_its_struct_matches_the_ctypes_mirror(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    declared = set(re.findall(r"^(?:int|long long)\s+(gi_\w+)\s*\(", hdr, flags=re.M))
    assert {"gi_grow_graphs", "gi_grow_state_words"} <= declared <= set(L.SIGNATURES)
    consts = {k: int(v) for k, v in re.findall(r"#define (GI_GROW_\w+)\s+(\d+)", hdr)}
    assert consts == {"GI_GROW_MAX_GROUPS": L.GROW_MAX_GROUPS, "GI_GROW_STATE_WORDS": L.GROW_STATE_WORDS,
                      "GI_GROW_ERR_ROUND": L.GROW_ERR_ROUND, "GI_GROW_ERR_CAPACITY": L.GROW_ERR_CAPACITY,
                      "GI_GROW_ERR_ACTION": L.GROW_ERR_ACTION, "GI_GROW_ERR_NNODES": L.GROW_ERR_NNODES}
    assert (GO.ERR_ROUND, GO.ERR_CAPACITY, GO.ERR_ACTION, GO.ERR_NNODES) == \
        (L.GROW_ERR_ROUND, L.GROW_ERR_CAPACITY, L.GROW_ERR_ACTION, L.GROW_ERR_NNODES)
    assert L.load().gi_grow_state_words(1000) == L.GROW_STATE_WORDS + 1000
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in L.GrowDesc._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "graphinvent_amd.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(gi_grow_desc));']
    src += [f'  printf("%zu\\n", offsetof(gi_grow_desc, {f}));' for f in fields]
    src += ['  return 0;', '}']
    cfile, exe = tmp_path / "grow.c", tmp_path / "grow"
    cfile.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(L.GrowDesc)
    assert got[1:] == [getattr(L.GrowDesc, f).offset for f in fields]
