"""What seeded generation costs at the GDB-13 shape (informational; bench.py measures the flagship training workload).

    python tools/bench_seeded.py [--batch 1000] [--iters 50] [--repeats 15] [--parent-lib PATH] [--out FILE]

GGNN with the reference defaults at h = 128 (seeded weights, untrained), B graphs, N = 13.  A few unseeded rounds
from the reference's initial state give a batch of partly grown graphs; that batch is kept FIXED as the input of every
timed round, so that every variant runs the same forward and draws the same actions (a seeded loop left to itself
grows larger graphs, whose forward costs more: that is the molecules' cost, not the step's).  The growth step works on
a copy of the tensors and its counters are zeroed before every round (one fill launch, in every variant), so no round
is frozen and every round writes out the same graphs.

Three measurements in one process, each variant timed with device events over `--iters` rounds, the variants
ALTERNATING inside each of `--repeats` repeats; per variant the median and the min / max over the repeats:

  step    the growth step alone (scan, apply, commit) — this tree's gi_grow_graphs, the seeded step with banks of
          S = 1, 64 and 4096 seeds, and, with --parent-lib (a libgraphinvent_amd.so built from the parent commit),
          that library's gi_grow_graphs on the same descriptor: the shared kernels must not have slowed down;
  round   a whole generation round (forward, draw, growth step): unseeded against seeded with S = 1, 64, 4096;
  init    gi_grow_seed_init alone, S = 64.

A seeded variant passes if its median lies inside the unseeded variant's min / max spread.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphinvent_amd import lib as L  # noqa: E402
from graphinvent_amd import synthetic  # noqa: E402
from graphinvent_amd.generator import _STATE_TENSORS, SeedBank, _Grower, new_state  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from graphinvent_amd.sampler import sample_actions_raw  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402
from tools.bench_generate import make_generator  # noqa: E402

DEV = "cuda"


def seed_bank(N, groups, Fe, S, dim_f_add, dim_f_conn, rng):
    """S chains of 1 .. N - 1 atoms (random features, node i bonded to node i - 1)."""
    Fn = sum(groups)
    nodes, edges = np.zeros((S, N, Fn), np.int8), np.zeros((S, N, N, Fe), np.int8)
    offs = np.concatenate([[0], np.cumsum(groups)[:-1]])
    for s in range(S):
        for i in range(1 + s % (N - 1)):
            for off, size in zip(offs, groups):
                nodes[s, i, off + rng.integers(size)] = 1
            if i:
                b = rng.integers(Fe)
                edges[s, i, i - 1, b] = edges[s, i - 1, i, b] = 1
    return SeedBank(torch.from_numpy(nodes).to(DEV), torch.from_numpy(edges).to(DEV), dim_f_add, dim_f_conn)


def event_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(variants, iters, repeats):
    """{name: {"median_ms", "min_ms", "max_ms"}} with the variants alternating inside every repeat."""
    for fn in variants.values():                                           # warm-up: code objects, workspaces
        event_ms(fn, 3)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(event_ms(fn, iters))
    return {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--prefill", type=int, default=6, help="unseeded rounds that grow the fixed input batch")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_seeded.py needs an MI355X"
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], hidden_node_features=128,
                          message_size=128)
    model = mpnn.GGNN(O.as_constants(dict(cfg, device=DEV)))
    model.load_state_dict(O.init_params(cfg, seed=0))
    model = model.to(DEV).eval()
    N, Fe = cfg["max_n_nodes"], cfg["n_edge_features"]
    groups = [sh["n_atom_types"], sh["n_formal_charge"]]
    from collections import namedtuple
    d = dict(device=DEV, max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=0,
             n_chirality=0, use_explicit_H=False, ignore_H=True, use_chirality=False, dim_nodes=[N, sum(groups)],
             dim_edges=[N, N, Fe], dim_f_add=[N, *groups, Fe], dim_f_conn=[N, Fe])
    c = namedtuple("CONSTANTS", sorted(d))(**d)
    B, Lc = a.batch, 32
    rng = np.random.default_rng(0)
    g = torch.Generator(device=DEV).manual_seed(0)

    with torch.no_grad():
        # the fixed input batch: a few unseeded rounds from the reference's initial state
        gen = make_generator(model, B, c, Lc)
        t = {name: getattr(gen, name) for name, _ in _STATE_TENSORS}
        state = new_state(B, 10 ** 9, DEV)
        grower = _Grower(t, c.dim_f_add, c.dim_f_conn, state)
        for _ in range(a.prefill):
            u = torch.rand(B, device=DEV, generator=g)
            grower.step(*sample_actions_raw(model(gen.nodes, gen.edges), gen.n_nodes, gen.edges, grower.A, uniform=u))
            state[0] = 0                                                   # (the generated rows are overwritten)
        fixed = {k: v.clone() for k, v in t.items()}
        u = torch.rand(B, device=DEV, generator=g)
        action, like, flags = sample_actions_raw(model(fixed["nodes"], fixed["edges"]), fixed["n_nodes"],
                                                 fixed["edges"], grower.A, uniform=u)
        written = int((action[1:, 0] == 2).sum() + (flags[1:] & 1).sum())

        def variant(S):
            """(step, round) closures of one variant on its own copy of the tensors; S = 0: unseeded."""
            w = {k: v.clone() for k, v in fixed.items()}
            st = new_state(B, 10 ** 9, DEV, seeded=S > 0)
            bank = seed_bank(N, groups, Fe, S, c.dim_f_add, c.dim_f_conn, rng) if S else None
            gs = torch.full((2 * B,), -1, dtype=torch.int32, device=DEV) if S else None
            gr = _Grower(w, c.dim_f_add, c.dim_f_conn, st, seeds=bank, gen_seed=gs)
            if S:
                gr.seed_init()
                for k in ("nodes", "edges", "n_nodes", "likelihoods"):    # ... and back to the fixed batch
                    w[k].copy_(fixed[k])

            fn = L.load().gi_grow_graphs_seeded if S else L.load().gi_grow_graphs
            extra = (C.byref(gr.seed_desc),) if S else ()

            def step():                      # the raw C call: the same host path for every variant of "step"
                st[:2].zero_()
                L.check(fn(C.byref(gr.desc), *extra, torch.cuda.current_stream().cuda_stream), "growth step")

            def round_():
                st[:2].zero_()
                gr.step(*sample_actions_raw(model(fixed["nodes"], fixed["edges"]), fixed["n_nodes"], fixed["edges"],
                                            gr.A, uniform=u))
            gr.step(action, like, flags)                                   # (fills the descriptor's per-round fields)
            return gr, st, step, round_

        made = {S: variant(S) for S in (0, 1, 64, 4096)}
        names = {0: "unseeded", 1: "seeded_S1", 64: "seeded_S64", 4096: "seeded_S4096"}
        steps = {names[S]: v[2] for S, v in made.items()}
        if a.parent_lib:
            parent = C.CDLL(os.path.abspath(a.parent_lib))
            parent.gi_grow_graphs.restype = C.c_int
            parent.gi_grow_graphs.argtypes = [C.POINTER(L.GrowDesc), C.c_void_p]
            gr0, st0 = made[0][0], made[0][1]

            def parent_step():
                st0[:2].zero_()
                L.check(parent.gi_grow_graphs(C.byref(gr0.desc), torch.cuda.current_stream().cuda_stream),
                        "parent gi_grow_graphs")
            steps = {"parent_unseeded": parent_step, **steps}
        out = {"batch": B, "N": N, "graphs_written_per_round": written, "iters": a.iters, "repeats": a.repeats,
               "parent_lib": bool(a.parent_lib)}
        out["step"] = alternate(steps, 4 * a.iters, a.repeats)
        out["round"] = alternate({names[S]: v[3] for S, v in made.items()}, a.iters, a.repeats)
        gr64 = made[64][0]
        out["init"] = alternate({"seed_init_S64": gr64.seed_init}, 4 * a.iters, a.repeats)
        for kind in ("step", "round"):
            base = out[kind]["unseeded"]
            for k, v in out[kind].items():
                v["inside_unseeded_spread"] = bool(base["min_ms"] <= v["median_ms"] <= base["max_ms"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
