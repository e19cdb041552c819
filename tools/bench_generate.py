"""A complete GraphGenerator.build_graphs at the GDB-13 shape (informational; bench.py measures the flagship training
workload and its "generation round" line keeps its meaning).

    python tools/bench_generate.py [--batch 1000] [--cap 24] [--builds 5] [--repeats 3] [--modes a,b,c,d]

GGNN with the reference defaults at h = 128 (seeded weights, untrained), batch_size graphs per build, the draws pinned
to the same uniforms [cap, B] in every mode.  Every mode gets a likelihood buffer of cap + 8 columns and stops at
`cap` rounds; an untrained model ends most graphs within a few rounds through invalid actions, so the round count is
printed and ms per round is the comparable figure.  Modes:
  a  the current best without the new step: blocking forward, sample_actions' index tuples and the reference's torch
     bookkeeping (oracle/callers_oracle.GeneratorOracle copy_terminated_graphs / apply_actions / reset_graphs);
  b  graphinvent_amd.generator.build_graphs with the blocking forward;
  c  the same with model.sync_free;
  d  the same with capture=True (one hipGraph per round).
Per mode: ms per build and per round, rounds, molecules/s, host synchronisations per round (counted with
torch.cuda.set_sync_debug_mode("warn") where this torch honours it; build_graphs' own polls and final wait are not
counted), graph_compact read-backs per round (ops.READBACKS), forwards per build (build_graphs enqueues up to
poll_every rounds past the last one; they change nothing but cost a forward each; mode d: replays, not counted) and
min / max over the repeats.  Mode d captures its graph in every build, and that capture is timed too.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import warnings
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphinvent_amd import ops, synthetic  # noqa: E402
from graphinvent_amd.generator import build_graphs  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from graphinvent_amd.sampler import sample_actions  # noqa: E402
from oracle import callers_oracle as CO  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402


def make_generator(model, B, c, Lc):
    gen = CO.GeneratorOracle(model, B, c, None)
    gen.likelihoods = torch.zeros(B, Lc, device="cuda")
    gen.generated_likelihoods = torch.zeros(2 * B, Lc, device="cuda")
    return gen


def torch_loop(gen, c, u):
    """Mode a: GeneratorOracle.build_graphs with sample_actions (the tuple layout) instead of the CPU draw."""
    n, r = 0, 0
    while n < gen.batch_size and r < u.shape[0]:
        add, conn, term, invalid, like = sample_actions(gen.model(gen.nodes, gen.edges), gen.n_nodes, gen.edges,
                                                        c.dim_f_add, c.dim_f_conn, uniform=u[r])
        gen.properly_terminated[n:(n + len(term))] = 1
        idc = torch.cat((term, invalid))
        idc = idc[idc != 0]
        n = gen.copy_terminated_graphs(idc, n, r, like)
        gen.apply_actions(add, conn, r, like)
        gen.reset_graphs(idc)
        r += 1
    gen.generation_rounds = r
    return n


FORWARDS = [0]


def run(mode, model, c, B, Lc, u, poll):
    gen = make_generator(model, B, c, Lc)
    FORWARDS[0] = 0
    model.sync_free = mode == "c"
    if mode == "a":
        n = torch_loop(gen, c, u)
    else:
        n = build_graphs(gen, c.dim_f_add, c.dim_f_conn, uniforms=u, poll_every=poll, capture=mode == "d")
    model.sync_free = False
    return n, gen.generation_rounds, gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=24)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--poll", type=int, default=8)
    ap.add_argument("--modes", default="a,b,c,d")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_generate.py needs an MI355X"
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], hidden_node_features=128,
                          message_size=128)
    model = mpnn.GGNN(O.as_constants(dict(cfg, device="cuda")))
    model.load_state_dict(O.init_params(cfg, seed=0))
    model = model.to("cuda").eval()
    model.register_forward_hook(lambda *_: FORWARDS.__setitem__(0, FORWARDS[0] + 1))
    N, Fe = cfg["max_n_nodes"], cfg["n_edge_features"]
    groups = [sh["n_atom_types"], sh["n_formal_charge"]]
    d = dict(device="cuda", max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=0,
             n_chirality=0, use_explicit_H=False, ignore_H=True, use_chirality=False, dim_nodes=[N, sum(groups)],
             dim_edges=[N, N, Fe], dim_f_add=[N, *groups, Fe], dim_f_conn=[N, Fe])
    c = namedtuple("CONSTANTS", sorted(d))(**d)
    B, Lc = a.batch, a.cap + 8
    u = torch.rand(a.cap, B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.ones(1, device="cuda").item()
    torch.cuda.set_sync_debug_mode(0)
    honoured = len(w) > 0

    out = {"batch": B, "round_cap": a.cap, "poll_every": a.poll, "builds_per_repeat": a.builds,
           "sync_debug_mode_honoured": honoured, "modes": {}}
    ref = None
    with torch.no_grad():
        for mode in a.modes.split(","):
            run(mode, model, c, B, Lc, u, a.poll)                         # warm-up (workspaces, caches, capture set-up)
            rb0 = dict(ops.READBACKS)
            torch.cuda.set_sync_debug_mode("warn" if honoured else 0)
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                n, rounds, gen = run(mode, model, c, B, Lc, u, a.poll)
            torch.cuda.set_sync_debug_mode(0)
            forwards = FORWARDS[0]
            syncs = sum("synchroniz" in str(x.message) for x in w)
            rb = {k: ops.READBACKS[k] - rb0[k] for k in rb0}
            got = (n, rounds, gen.generated_n_nodes.cpu(), gen.generated_edges.cpu())
            if ref is None:
                ref = got
            same = got[:2] == ref[:2] and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
            times = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.builds):
                    run(mode, model, c, B, Lc, u, a.poll)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / a.builds * 1e3)
            ms = float(np.median(times))
            out["modes"][mode] = {
                "ms_per_build": round(ms, 3), "rounds": rounds, "ms_per_round": round(ms / rounds, 3),
                "molecules": n, "molecules_per_s": round(n / ms * 1e3, 1),
                "forwards_per_build": forwards if mode != "d" else None,
                "ms_per_build_min_max": [round(min(times), 3), round(max(times), 3)],
                "host_syncs_per_round": round(syncs / rounds, 2) if honoured else None,
                "compact_readbacks_per_round": {k: round(v / rounds, 2) for k, v in rb.items()},
                "same_graphs_as_mode_a": bool(same)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
