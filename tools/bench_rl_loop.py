"""A complete GraphGeneratorRL.build_graphs with its loss backward (informational; bench.py measures the flagship
training workload).

    python tools/bench_rl_loop.py [--batch 1000] [--builds 3] [--repeats 3] [--poll 1] [--models golden,default]

Two modes on the same pinned uniforms [64, B]:
  a  what INTEGRATION.md recommended before build_graphs_rl: both forwards with grad, sample_actions_rl's index tuples
     and the reference's torch bookkeeping (tests/rl_callers.GeneratorRLOracle with the HIP sampler);
  b  graphinvent_amd.generator.build_graphs_rl.
Two models: "golden" = the drop-in GGNN with tests/golden/golden_generator.npz's trained weights (its golden RL run
took 22 rounds for 100 graphs) and the perturbed prior of the RL goldens; "default" = the GGNN with the reference
defaults at the GDB-13 shape, seeded and untrained (most graphs end within a few rounds through invalid actions).
Both loops get 64 likelihood columns.  Per model and mode: ms per build, rounds, ms per round, host synchronisations
per round (torch.cuda.set_sync_debug_mode("warn") where this torch honours it; build_graphs_rl's own polls and final
wait are not counted), ms of the backward of Workflow.compute_loss_component (random scores), and whether the graphs
equal mode a's.  Prints one JSON line."""
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

from graphinvent_amd import synthetic  # noqa: E402
from graphinvent_amd.generator import build_graphs_rl  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from graphinvent_amd.sampler import sample_actions_rl  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402
from tests import rl_callers as RL  # noqa: E402
from tests.golden import ref_callers as RC  # noqa: E402

LC = 64


def gen_constants(N, groups, Fe):
    d = dict(device="cuda", max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=0,
             n_chirality=0, use_explicit_H=False, ignore_H=True, use_chirality=False, dim_nodes=[N, sum(groups)],
             dim_edges=[N, N, Fe], dim_f_add=[N, *groups, Fe], dim_f_conn=[N, Fe])
    return namedtuple("CONSTANTS", sorted(d))(**d)


def models(which):
    if which == "golden":
        G = np.load(os.path.join(ROOT, "tests", "golden", "golden_generator.npz"))
        cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
        c = RC.as_constants(RC.constants_dict("cuda", cfg, "/nonexistent", batch_size=int(G["batch"]), epochs=1))
        agent = mpnn.GGNN(constants=c)
        agent.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    else:
        sh = synthetic.SHAPES["gdb13"]
        cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
        agent = mpnn.GGNN(O.as_constants(dict(cfg, device="cuda")))
        agent.load_state_dict(O.init_params(cfg, seed=0))
        c = gen_constants(sh["max_n_nodes"], [sh["n_atom_types"], sh["n_formal_charge"]], sh["n_edge_features"])
    prior = RL.perturbed_prior(agent)
    return c, agent.to("cuda").train(), prior.to("cuda").eval()


def make_generator(agent, prior, B, c, sampler=None):
    gen = RL.GeneratorRLOracle(agent, prior, B, c, sampler=sampler)
    for name in ("agent_likelihoods", "prior_likelihoods"):
        setattr(gen, name, torch.zeros(B, LC, device="cuda"))
    for name in ("generated_agent_likelihoods", "generated_prior_likelihoods"):
        setattr(gen, name, torch.zeros(2 * B, LC, device="cuda"))
    return gen


def run(mode, agent, prior, c, B, u, poll):
    if mode == "a":
        r = [0]

        def draw(agent_logits, prior_logits, n_nodes, edges):
            r[0] += 1
            return sample_actions_rl(agent_logits, prior_logits, n_nodes, edges, c.dim_f_add, c.dim_f_conn,
                                     uniform=u[r[0] - 1])
        gen = make_generator(agent, prior, B, c, draw)
        n = gen.build_graphs()
        gen.generation_rounds = gen.rounds
    else:
        gen = make_generator(agent, prior, B, c)
        n = build_graphs_rl(gen, c.dim_f_add, c.dim_f_conn, uniforms=u, poll_every=poll)
    return n, gen


def loss_of(gen, B, scores):
    a_ll, p_ll = gen.loglikelihoods()
    return torch.mean(RL.compute_loss_component(scores, a_ll, p_ll, torch.ones(B, device="cuda"), 20.0))


def zero_grads(*ms):
    for m in ms:
        for p in m.parameters():
            p.grad = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--poll", type=int, default=1)
    ap.add_argument("--models", default="golden,default")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_rl_loop.py needs an MI355X"
    B = a.batch
    u = torch.rand(LC, B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    scores = torch.rand(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.ones(1, device="cuda").item()
    torch.cuda.set_sync_debug_mode(0)
    honoured = len(w) > 0

    out = {"batch": B, "poll_every": a.poll, "builds_per_repeat": a.builds, "repeats": a.repeats,
           "sync_debug_mode_honoured": honoured, "models": {}}
    for which in a.models.split(","):
        c, agent, prior = models(which)
        res, ref = {}, None
        for mode in ("a", "b"):
            zero_grads(agent, prior)
            n, gen = run(mode, agent, prior, c, B, u, a.poll)             # warm-up
            loss_of(gen, B, scores).backward()
            torch.cuda.set_sync_debug_mode("warn" if honoured else 0)
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                n, gen = run(mode, agent, prior, c, B, u, a.poll)
            torch.cuda.set_sync_debug_mode(0)
            syncs = sum("synchroniz" in str(x.message) for x in w)
            rounds = gen.generation_rounds
            got = (n, rounds, gen.generated_n_nodes.cpu(), gen.generated_edges.cpu())
            del gen
            if ref is None:
                ref = got
            same = got[:2] == ref[:2] and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
            fwd, bwd = [], []
            for _ in range(a.repeats):
                tf = tb = 0.0
                for _ in range(a.builds):
                    zero_grads(agent, prior)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, gen = run(mode, agent, prior, c, B, u, a.poll)
                    loss = loss_of(gen, B, scores)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    loss.backward()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    tf += t1 - t0
                    tb += t2 - t1
                    del gen, loss
                fwd.append(tf / a.builds * 1e3)
                bwd.append(tb / a.builds * 1e3)
            ms = float(np.median(fwd))
            res[mode] = {"ms_per_build": round(ms, 3), "rounds": rounds, "ms_per_round": round(ms / rounds, 3),
                         "molecules": n, "ms_per_build_min_max": [round(min(fwd), 3), round(max(fwd), 3)],
                         "host_syncs_per_round": round(syncs / rounds, 2) if honoured else None,
                         "backward_ms": round(float(np.median(bwd)), 3), "same_graphs_as_mode_a": bool(same)}
        res["saved_ms_per_round"] = round(res["a"]["ms_per_round"] - res["b"]["ms_per_round"], 3)
        out["models"][which] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
