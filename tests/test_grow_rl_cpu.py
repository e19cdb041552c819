"""CPU: the boundary of the RL growth step (gi_grow_graphs_rl, gi_grow_traj_gather / gi_grow_traj_scatter) and of
graphinvent_amd.generator.build_graphs_rl: the entry points are declared, exported and bound; the header's
gi_grow_rl_desc matches its ctypes mirror; the loop refuses what the kernels cannot take, with build_graphs'
exceptions, before anything reaches the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from graphinvent_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"gi_grow_graphs_rl", "gi_grow_rl_state_words", "gi_grow_traj_gather", "gi_grow_traj_scatter"}


def test_rl_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    declared = set(re.findall(r"^(?:int|long long)\s+(gi_\w+)\s*\(", hdr, flags=re.M))
    assert ENTRIES <= declared <= set(L.SIGNATURES)
    lib = L.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.gi_grow_rl_state_words(1000) == L.GROW_STATE_WORDS + 2000
    assert lib.gi_grow_rl_state_words(-1) < 0
    assert lib.gi_abi_version() == L.ABI_VERSION == 18
    from graphinvent_amd.generator import new_state
    assert new_state(7, 7, "cpu", rl=True).numel() == lib.gi_grow_rl_state_words(7)
    assert new_state(7, 7, "cpu").numel() == lib.gi_grow_state_words(7)


def test_header_rl_desc_matches_the_ctypes_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in L.GrowRlDesc._fields_]
    base = [f for f, _ in L.GrowDesc._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "graphinvent_amd.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(gi_grow_rl_desc));']
    src += [f'  printf("%zu\\n", offsetof(gi_grow_rl_desc, {f}));' for f in fields]
    src += [f'  printf("%zu\\n", offsetof(gi_grow_rl_desc, base.{f}));' for f in base]
    src += ['  return 0;', '}']
    cfile, exe = tmp_path / "grow_rl.c", tmp_path / "grow_rl"
    cfile.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(L.GrowRlDesc)
    assert got[1:1 + len(fields)] == [getattr(L.GrowRlDesc, f).offset for f in fields]
    assert got[1 + len(fields):] == [getattr(L.GrowDesc, f).offset for f in base]    # base is the first member
    assert L.GrowRlDesc.base.offset == 0


def _gen(B=4, N=3, Fn=5, Fe=2, Lc=6, **over):
    """GraphGeneratorRL's tensors (allocate_graph_tensors: C = 2 B) on the host, with overrides."""
    Cg = 2 * B
    t = dict(nodes=torch.zeros(B, N, Fn), edges=torch.zeros(B, N, N, Fe), n_nodes=torch.zeros(B, dtype=torch.int8),
             agent_likelihoods=torch.zeros(B, Lc), prior_likelihoods=torch.zeros(B, Lc),
             generated_nodes=torch.zeros(Cg, N, Fn), generated_edges=torch.zeros(Cg, N, N, Fe),
             generated_n_nodes=torch.zeros(Cg, dtype=torch.int8), generated_agent_likelihoods=torch.zeros(Cg, Lc),
             generated_prior_likelihoods=torch.zeros(Cg, Lc), properly_terminated=torch.zeros(Cg, dtype=torch.int8))
    t.update(over)

    class Gen:
        agent_model = prior_model = None
        batch_size = B
    gen = Gen()
    for k, v in t.items():
        setattr(gen, k, v)
    return gen


def _call(gen, dim_f_add=(3, 3, 2, 2), dim_f_conn=(3, 2), **kw):
    from graphinvent_amd.generator import build_graphs_rl
    return build_graphs_rl(gen, dim_f_add, dim_f_conn, **kw)


def test_build_graphs_rl_refuses_a_cpu_generator():
    with pytest.raises(RuntimeError, match="CUDA"):
        _call(_gen())


@pytest.mark.parametrize("name,bad,exc", [
    ("n_nodes", torch.zeros(4, dtype=torch.int32), TypeError),
    ("edges", torch.zeros(4, 3, 3, 2, dtype=torch.float64), TypeError),
    ("agent_likelihoods", torch.zeros(4, 6, dtype=torch.float64), TypeError),
    ("prior_likelihoods", torch.zeros(4, 6, dtype=torch.float16), TypeError),
    ("generated_prior_likelihoods", torch.zeros(8, 6, dtype=torch.float64), TypeError),
    ("properly_terminated", torch.zeros(8, dtype=torch.bool), TypeError),
    ("agent_likelihoods", torch.zeros(6, 4).t(), ValueError),                  # not contiguous
    ("prior_likelihoods", torch.zeros(6, 4).t(), ValueError),
    ("generated_edges", torch.zeros(8, 3, 3, 3), ValueError),                   # Fe mismatch
    ("generated_agent_likelihoods", torch.zeros(8, 5), ValueError),             # L mismatch
    ("generated_prior_likelihoods", torch.zeros(8, 5), ValueError),
    ("prior_likelihoods", torch.zeros(4, 7), ValueError),
    ("properly_terminated", torch.zeros(7, dtype=torch.int8), ValueError),      # C mismatch
    ("n_nodes", torch.zeros(5, dtype=torch.int8), ValueError),
])
def test_build_graphs_rl_refuses_wrong_dtypes_and_shapes(name, bad, exc):
    with pytest.raises(exc):
        _call(_gen(**{name: bad}))


@pytest.mark.parametrize("dim_f_add,dim_f_conn", [((3, 3, 3, 2), (3, 2)), ((3, 3, 2, 3), (3, 2)),
                                                   ((4, 3, 2, 2), (4, 2)), ((3, 3, 2, 2), (3, 3))])
def test_build_graphs_rl_checks_the_add_layout(dim_f_add, dim_f_conn):
    with pytest.raises(ValueError):
        _call(_gen(), dim_f_add, dim_f_conn)


def test_build_graphs_rl_refuses_a_bad_poll_interval():
    with pytest.raises(ValueError, match="poll_every"):
        _call(_gen(), poll_every=0)
