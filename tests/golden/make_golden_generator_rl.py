"""Golden vectors for the RL generation loop, produced in the build container by the UNMODIFIED reference
``GraphGeneratorRL.build_graphs`` (GraphGeneratorRL.py:109-172 and what it calls) and ``Workflow.compute_loss_component``
(Workflow.py:862-898), with the reference's own ``gnn`` on CPU.

The set-up is ``Workflow.learning_step``'s (:569-598): the agent (the small GGNN whose trained weights
tests/golden/golden_generator.npz stores) in ``train()`` mode and the prior, a weight-perturbed copy (tests/rl_callers.py ``perturbed_prior``,
regenerated from its seed, checked against a stored digest), both running with grad; the loop's one random draw is pinned to ``InverseCdfDraws`` (tests/golden/ref_callers.py ``pin_multinomial``).
The file holds the generated graphs, the agent and prior log-likelihoods computed as ``sample()`` does (:86-92), the
loss ``mean(compute_loss_component(...))`` with fixed scores and uniqueness (sigma = 20), and the gradients of that
loss for the agent's and the prior's parameters.  The gradients are stored as fp16 scaled by each tensor's largest
magnitude (tests/rl_callers.py ``pack_grad``): within 2.5e-4 of that magnitude, and half the bytes of fp32.

Before anything is written the restatement tests/rl_callers.py runs on the same models and draws and must reproduce
the unmodified methods BIT FOR BIT (graphs, log-likelihoods, loss, every gradient)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import callers_oracle as CO            # noqa: E402
from oracle import ggnn_oracle as O                # noqa: E402
from tests import rl_callers as RL                 # noqa: E402
from tests.golden import ref_callers as RC         # noqa: E402

BATCH, SIGMA = 100, 20.0


def load_reference(consts):
    WF, _ = RC.load("reference", consts)
    sys.modules.pop("GraphGeneratorRL", None)                  # ref_callers stubs it; the real class is under test
    sys.path.insert(0, RC.REF)
    try:
        import GraphGeneratorRL
        import gnn.mpnn
    finally:
        sys.path.remove(RC.REF)
    assert GraphGeneratorRL.__file__.startswith(RC.REF) and gnn.mpnn.__file__.startswith(RC.REF)
    return WF, GraphGeneratorRL, gnn.mpnn


def models(mpnn, consts, G):
    agent = mpnn.GGNN(consts)
    agent.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    prior = RL.perturbed_prior(agent)
    return agent.train(), prior.eval()


def fixed_scores():
    rng = np.random.default_rng(9)
    scores = rng.random(BATCH).astype(np.float32)
    uniqueness = (rng.random(BATCH) > 0.15).astype(np.float32)
    return torch.from_numpy(scores), torch.from_numpy(uniqueness)


def run(make_generator, agent, prior, draw_seed, loss_component):
    agent.zero_grad(set_to_none=True)
    prior.zero_grad(set_to_none=True)
    draw = CO.InverseCdfDraws(draw_seed, BATCH)
    RC.pin_multinomial(draw)
    gen = make_generator(agent, prior, draw)
    n = gen.build_graphs()
    a_ll = torch.log(torch.sum(gen.generated_agent_likelihoods, dim=1)[:BATCH])       # sample(), :86-92
    p_ll = torch.log(torch.sum(gen.generated_prior_likelihoods, dim=1)[:BATCH])
    scores, uniqueness = fixed_scores()
    loss = torch.mean(loss_component(scores, a_ll, p_ll, uniqueness))                  # Workflow.py:748-754
    loss.backward()
    return dict(n_generated=n, rounds=draw.round, margin=draw.margin, nodes=gen.generated_nodes.numpy(),
                edges=gen.generated_edges.numpy(), n_nodes=gen.generated_n_nodes.numpy(),
                terminated=gen.properly_terminated.numpy(), agent_ll=a_ll.detach().numpy(),
                prior_ll=p_ll.detach().numpy(), loss=float(loss),
                grad_agent={k: p.grad.clone() for k, p in agent.named_parameters()},
                grad_prior={k: p.grad.clone() for k, p in prior.named_parameters()})


def main():
    assert RC.have_reference()
    G = np.load(os.path.join(HERE, "golden_generator.npz"))
    cfg_items = {str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])}
    consts = RC.as_constants(dict(RC.constants_dict("cpu", O.make_config(**cfg_items), "/nonexistent",
                                                    batch_size=BATCH, epochs=1), sigma=SIGMA))
    WF, GGRL, mpnn = load_reference(consts)
    agent, prior = models(mpnn, consts, G)
    fake_wf = types.SimpleNamespace(constants=consts)

    def ref_loss(s, a, p, u):
        return WF.Workflow.compute_loss_component(fake_wf, scores=s, agent_loglikelihoods=a,
                                                  prior_loglikelihoods=p, uniqueness=u)

    def ref_generator(a, p, draw):
        gen = GGRL.GraphGeneratorRL(model=a, batch_size=BATCH)
        gen.agent_model, gen.prior_model = a, p                        # what sample() sets (:76-77)
        return gen

    draw_seed = 0
    while True:
        ref = run(ref_generator, agent, prior, draw_seed, ref_loss)
        if ref["margin"] > 2e-5:
            break
        draw_seed += 1
    mine = run(lambda a, p, draw: RL.GeneratorRLOracle(a, p, BATCH, consts, draw), agent, prior, draw_seed,
               lambda s, a, p, u: RL.compute_loss_component(s, a, p, u, SIGMA))
    for k in ("n_generated", "rounds", "loss"):
        assert ref[k] == mine[k], (k, ref[k], mine[k])
    for k in ("nodes", "edges", "n_nodes", "terminated", "agent_ll", "prior_ll"):
        assert np.array_equal(ref[k], mine[k]), k
    for side in ("grad_agent", "grad_prior"):
        for k in ref[side]:
            assert torch.equal(ref[side][k], mine[side][k]), (side, k)
    print("GraphGeneratorRL.build_graphs + compute_loss_component: restatement == unmodified, bit for bit;",
          ref["n_generated"], "graphs in", ref["rounds"], "rounds, margin", ref["margin"], "draw seed", draw_seed,
          "loss", ref["loss"])
    scores, uniqueness = fixed_scores()
    blob = dict(draw_seed=draw_seed, batch=BATCH, sigma=SIGMA, n_generated=ref["n_generated"], rounds=ref["rounds"],
                margin=ref["margin"], nodes=ref["nodes"].astype(np.int8), edges=ref["edges"].astype(np.int8),
                n_nodes=ref["n_nodes"], terminated=ref["terminated"], agent_ll=ref["agent_ll"],
                prior_ll=ref["prior_ll"], loss=ref["loss"], scores=scores.numpy(), uniqueness=uniqueness.numpy(),
                cfg_keys=G["cfg_keys"], cfg_vals=G["cfg_vals"])
    blob["prior_digest"] = RL.weight_digest(prior)          # the agent's weights are golden_generator.npz's w::*
    for prefix, grads in (("ga::", ref["grad_agent"]), ("gp::", ref["grad_prior"])):
        for k, v in grads.items():
            blob.update(RL.pack_grad(prefix + k, v.numpy()))
    np.savez_compressed(os.path.join(HERE, "golden_generator_rl.npz"), **blob)


if __name__ == "__main__":
    with RC.isolated():
        main()
