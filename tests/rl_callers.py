"""Test infrastructure: restatement of the reference's RL generation loop, ``GraphGeneratorRL`` (GraphGeneratorRL.py;
file:line relative to the reference's ``graphinvent/``), and of ``Workflow.compute_loss_component`` (Workflow.py:862-898).

``GeneratorRLOracle`` reuses ``oracle.callers_oracle.GeneratorOracle`` for ``initialize_graph_batch`` and the action
application, and restates what the RL class changes: two likelihood buffers (agent and prior), both models run with
grad on the same graphs every round (:131-132), and ``get_actions`` returning both models' probabilities of the action
drawn from the agent (:521-633).  ``sampler`` selects how a round's step runs:

* ``None``: the reference's sequence — ``softmax`` of both outputs, the draw (``draw``, e.g. ``InverseCdfDraws``) on
  the agent's APD, ``oracle.sampler_oracle.get_actions`` on the drawn index, and the likelihoods gathered from the
  APDs with autograd (what ``agent_apds[one_hot == 1]`` differentiates to);
* a callable ``(agent_logits, prior_logits, n_nodes, edges) -> get_actions tuple``: e.g. a wrapper of
  ``graphinvent_amd.sampler.sample_actions_rl`` (the two-line replacement of INTEGRATION.md).

tests/golden/make_golden_generator_rl.py checks this restatement against the UNMODIFIED ``GraphGeneratorRL`` bit for
bit before it writes tests/golden/golden_generator_rl.npz."""
from __future__ import annotations

import numpy as np
import torch

from oracle import callers_oracle as CO
from oracle import sampler_oracle as SO


def get_actions_rl(agent_apds, prior_apds, idx, n_nodes, edges, dim_f_add, dim_f_conn, device="cpu"):
    """GraphGeneratorRL.get_actions (:521-633) after the draw: the index tuples of the sampler oracle, and both
    likelihoods gathered at the drawn index (differentiable like ``apds[one_hot == 1]``)."""
    out = SO.get_actions(agent_apds.detach().cpu().numpy(), idx, n_nodes, edges, dim_f_add, dim_f_conn)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(device)
    rows = torch.arange(agent_apds.shape[0], device=agent_apds.device)
    i = torch.as_tensor(idx, device=agent_apds.device)
    return (tuple(t(x) for x in out["add"]), tuple(t(x) for x in out["conn"]), t(out["term"]), t(out["invalid"]),
            agent_apds[rows, i], prior_apds[rows, i])


class GeneratorRLOracle(CO.GeneratorOracle):
    def __init__(self, agent_model, prior_model, batch_size, constants, draw=None, sampler=None):   # :27-53
        self.agent_model, self.prior_model, self.sampler = agent_model, prior_model, sampler
        super().__init__(None, batch_size, constants, draw)

    def allocate_graph_tensors(self):                                     # :177-224
        super().allocate_graph_tensors()
        c, B = self.c, self.batch_size
        shape = (B, c.max_n_nodes * 2)
        self.agent_likelihoods = torch.zeros(shape, device=c.device)
        self.prior_likelihoods = torch.zeros(shape, device=c.device)
        self.generated_agent_likelihoods = torch.zeros((2 * B, shape[1]), device=c.device)
        self.generated_prior_likelihoods = torch.zeros((2 * B, shape[1]), device=c.device)

    def get_actions(self, agent_logits, prior_logits):
        if self.sampler is not None:
            return self.sampler(agent_logits, prior_logits, self.n_nodes, self.edges)
        softmax = torch.nn.Softmax(dim=1)                                 # :115, 131-132
        agent_apd, prior_apd = softmax(agent_logits), softmax(prior_logits)
        idx = self.draw(agent_apd.detach().cpu().numpy())
        return get_actions_rl(agent_apd, prior_apd, idx, self.n_nodes.cpu().numpy(), self.edges.cpu().numpy(),
                              self.c.dim_f_add, self.c.dim_f_conn, self.c.device)

    def build_graphs(self):                                               # :109-172
        n_generated_so_far = 0
        self.rounds = 0
        while n_generated_so_far < self.batch_size:
            agent_logits = self.agent_model(self.nodes, self.edges)
            prior_logits = self.prior_model(self.nodes, self.edges)
            add, conn, term, invalid, agent_like, prior_like = self.get_actions(agent_logits, prior_logits)
            self.properly_terminated[n_generated_so_far:(n_generated_so_far + len(term))] = 1    # :141
            termination_idc = torch.cat((term, invalid))
            termination_idc = termination_idc[termination_idc != 0]       # :147
            n_generated_so_far = self.copy_terminated_graphs(termination_idc, n_generated_so_far, self.rounds,
                                                             agent_like, prior_like)
            self.apply_actions(add, conn, self.rounds, agent_like, prior_like)
            self.reset_graphs(termination_idc)
            self.rounds += 1
        return n_generated_so_far

    def apply_actions(self, add, conn, generation_round, agent_like, prior_like):   # :226-346
        # the graph edits are GraphGenerator's (same code at :264-318); likelihoods go to the two RL buffers
        super().apply_actions(add, conn, generation_round, agent_like.detach())
        for batch in (add[0].long(), conn[0].long()):                     # :316-317, :343-344
            self.agent_likelihoods[batch, generation_round] = agent_like[batch]
            self.prior_likelihoods[batch, generation_round] = prior_like[batch]

    def copy_terminated_graphs(self, terminate_idc, n_graphs_generated, generation_round, agent_like, prior_like):
        self.agent_likelihoods[terminate_idc, generation_round] = agent_like[terminate_idc]       # :378-379
        self.prior_likelihoods[terminate_idc, generation_round] = prior_like[terminate_idc]
        n = len(terminate_idc)
        lo, hi = n_graphs_generated, n_graphs_generated + n
        self.generated_nodes[lo:hi] = self.nodes[terminate_idc]
        self.generated_edges[lo:hi] = self.edges[terminate_idc]
        self.generated_n_nodes[lo:hi] = self.n_nodes[terminate_idc]
        self.generated_agent_likelihoods[lo:hi] = self.agent_likelihoods[terminate_idc]
        self.generated_prior_likelihoods[lo:hi] = self.prior_likelihoods[terminate_idc]
        return n_graphs_generated + n

    def reset_graphs(self, idc):                                          # :453-498
        if len(idc) > 0:
            self.agent_likelihoods[idc] = torch.zeros((len(idc), self.agent_likelihoods.shape[1]),
                                                      device=self.c.device)
            self.prior_likelihoods[idc] = torch.zeros((len(idc), self.prior_likelihoods.shape[1]),
                                                      device=self.c.device)
        super().reset_graphs(idc)

    def loglikelihoods(self):                                             # sample(), :86-92
        B = self.batch_size
        return (torch.log(torch.sum(self.generated_agent_likelihoods, dim=1)[:B]),
                torch.log(torch.sum(self.generated_prior_likelihoods, dim=1)[:B]))


def get_actions_rl_torch(agent_apds, prior_apds, n_nodes, edges, dim_f_add, dim_f_conn):
    """The reference's device sequence of GraphGeneratorRL.get_actions / get_invalid_actions (:521-720) in torch ops:
    ``Multinomial`` draw, boolean-mask gathers, ``nonzero`` index tuples and the validity rules (for timing the step
    the HIP kernel replaces; tools/bench_rl.py)."""
    B = agent_apds.shape[0]
    f_add_size = int(np.prod(dim_f_add))
    one_hot = torch.distributions.Multinomial(1, probs=agent_apds).sample()
    f_add = one_hot[:, :f_add_size].reshape(B, *dim_f_add)
    f_conn = one_hot[:, f_add_size:-1].reshape(B, *dim_f_conn)
    agent_like, prior_like = agent_apds[one_hot == 1], prior_apds[one_hot == 1]
    add = list(torch.nonzero(f_add, as_tuple=True))
    conn = list(torch.nonzero(f_conn, as_tuple=True))
    term = torch.nonzero(one_hot[:, -1]).view(-1)
    nn_add, nn_conn = n_nodes[add[0]], n_nodes[conn[0]]
    add.append(nn_add)
    conn.append(nn_conn - 1)

    def setop(a, b, keep):                         # set difference (counts == 1) / intersection (counts > 1)
        u, c = torch.cat((a, b)).squeeze(1).unique(return_counts=True)
        return u[keep(c)].unsqueeze(1)
    empty = torch.nonzero(nn_add == 0)
    invalid_add = setop(torch.nonzero(add[1] >= nn_add), empty, lambda c: c == 1)
    invalid_add_empty = setop(torch.nonzero(add[1] != nn_add), empty, lambda c: c > 1)
    invalid_madd = torch.nonzero(add[-1] >= dim_f_add[0])
    invalid_conn = torch.nonzero(conn[1] >= nn_conn)
    invalid_conn_nonex = torch.nonzero(nn_conn == 0)
    invalid_sconn = torch.nonzero(conn[1] == conn[3])
    invalid_dconn = torch.nonzero(torch.sum(edges, dim=-1)[conn[0].long(), conn[1].long(), conn[-1].long()] == 1)
    invalid = torch.unique(torch.cat((add[0][invalid_add], add[0][invalid_add_empty], conn[0][invalid_conn],
                                      conn[0][invalid_conn_nonex], conn[0][invalid_sconn], conn[0][invalid_dconn],
                                      add[0][invalid_madd])))
    needs_reset = torch.unique(torch.cat((invalid_madd, empty)))
    add[-1][needs_reset] = 0
    return tuple(add), tuple(conn), term, invalid, agent_like, prior_like


def perturbed_prior(agent, rel=0.02, seed=5):
    """The prior of the RL goldens: a deepcopy of the agent with every tensor moved by ``rel`` x its spread of
    seeded normal noise (torch's CPU generator, so the same weights on every box; the goldens carry a digest)."""
    import copy
    prior = copy.deepcopy(agent)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in prior.parameters():
            scale = float(p.std() if p.numel() > 1 else p.abs().max())
            p.add_((rel * scale * torch.randn(p.shape, generator=g)).to(p.device))
    return prior


def weight_digest(model):
    """Per parameter: (sum, sum of squares) in float64."""
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().pow(2).sum())]
                     for p in model.parameters()])


def pack_grad(key, g):
    """A gradient tensor as golden_generator_rl.npz stores it: fp16 of g / max|g| under ``key``, the scale under
    ``"gs::" + key`` (every element within 2**-12 of max|g| of the fp32 value)."""
    scale = np.float32(np.abs(g).max() or 1.0)
    return {key: (g / scale).astype(np.float16), "gs::" + key: scale}


def unpack_grad(G, key):
    return torch.from_numpy(G[key].astype(np.float64) * float(G["gs::" + key]))


def grad_errors(model, G, prefix):
    """(global relative L2, worst per-tensor max-abs relative) of ``model``'s gradients against the stored ones."""
    num = den = worst = 0.0
    for k, p in model.named_parameters():
        ref = unpack_grad(G, prefix + k)
        got = p.grad.detach().double().cpu()
        num += float((got - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
        worst = max(worst, float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)))
    return (num / den) ** 0.5, worst


def compute_loss_component(scores, agent_loglikelihoods, prior_loglikelihoods, uniqueness, sigma):
    """Workflow.compute_loss_component (:862-898)."""
    difference = agent_loglikelihoods - (prior_loglikelihoods + sigma * scores)
    return difference * difference * (uniqueness != 0).int()
