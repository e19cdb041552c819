"""-m gpu: the RL sampling step (gi_sample_actions_rl / gi_sample_likelihood_bwd, graphinvent_amd.sampler
.sample_actions_rl) against the RL oracle (pinned to the unmodified reference by tests/test_sampler_rl_cpu.py):
  * the fixture: draws bracket u in the fp64 CDF, decode bit-exact, the reference's own draws reproduced exactly, both
    likelihoods to 1e-6, the reference's autograd gradients of both logits tensors;
  * agreement with gi_sample_actions bit for bit on the agent side;
  * the backward against torch autograd of softmax(l).gather(idx) up to the row limit, pitched rows, a prior without
    grad, one tensor passed as both, a None upstream gradient;
  * the restated GraphGeneratorRL loop on the drop-in GGNN: the reference's graphs, log-likelihoods and gradients."""
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import sampler
from oracle import callers_oracle as CO
from oracle import ggnn_oracle as O
from oracle import sampler_oracle as SO
from tests import rl_callers as RL
from tests.golden import ref_callers as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _flat_index(action, N, A, Fe):
    kind, node, rem = action[:, 0], action[:, 1], action[:, 2]
    return np.where(kind == 0, node * A + rem, np.where(kind == 1, N * A + node * Fe + rem, N * A + N * Fe))


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "golden_sampler_rl.npz"))
    dim_f_add, dim_f_conn = g["dim_f_add"].tolist(), g["dim_f_conn"].tolist()
    return g, dim_f_add, dim_f_conn, int(np.prod(dim_f_add[1:]))


@pytest.mark.parametrize("edge_dtype", [torch.float32, torch.int8])
def test_rl_sampler_on_the_reference_fixture(golden_dir, edge_dtype):
    g, dim_f_add, dim_f_conn, A = _fixture(golden_dir)
    N, Fe = dim_f_conn
    la, lp = (torch.from_numpy(g[k]).to(DEV) for k in ("agent_logits", "prior_logits"))
    n_nodes = torch.from_numpy(g["n_nodes"]).to(DEV)
    edges = torch.from_numpy(g["edges"]).to(DEV).to(edge_dtype)
    B = la.shape[0]
    pa, pp = SO.softmax_rows(g["agent_logits"]), SO.softmax_rows(g["prior_logits"])
    cdf = np.cumsum(pa, axis=1)
    gen = torch.Generator(device=DEV).manual_seed(7)
    rows = np.arange(B)
    for trial in range(6):
        u = torch.rand(B, device=DEV, generator=gen)
        if trial == 0:
            u[:4] = torch.tensor([0.0, 0.999999, 0.5, 1e-7], device=DEV)
        action, like_a, like_p, flags, idx, lse = sampler.sample_actions_rl_raw(la, lp, n_nodes, edges, A, u)
        k = _flat_index(action.cpu().numpy(), N, A, Fe)
        assert np.array_equal(k, idx.cpu().numpy())
        un = u.cpu().numpy().astype(np.float64)
        lo = np.where(k > 0, cdf[rows, np.maximum(k - 1, 0)], 0.0)
        assert np.all(lo - 1e-5 <= un) and np.all(un < cdf[rows, k] + 1e-5), "draw is not the inverse CDF of u"
        out = sampler.sample_actions_rl(la, lp, n_nodes, edges, dim_f_add, dim_f_conn, uniform=u)
        ref = SO.get_actions(pa, k, g["n_nodes"], g["edges"], dim_f_add, dim_f_conn)
        for j in range(6):
            assert np.array_equal(out[0][j].cpu().numpy(), ref["add"][j]), f"add[{j}]"
        for j in range(4):
            assert np.array_equal(out[1][j].cpu().numpy(), ref["conn"][j]), f"conn[{j}]"
        assert np.array_equal(out[2].cpu().numpy(), ref["term"])
        assert np.array_equal(out[3].cpu().numpy(), ref["invalid"])
        assert np.abs(out[4].cpu().numpy() - pa[rows, k]).max() < 1e-6
        assert np.abs(out[5].cpu().numpy() - pp[rows, k]).max() < 1e-6
        assert np.all(like_a.cpu().numpy() > 0) and np.all(out[4].cpu().numpy() > 0)
        lse_ref = np.stack([np.log(np.exp(g[n].astype(np.float64)).sum(1)) for n in ("agent_logits", "prior_logits")], 1)
        assert np.abs(lse.cpu().numpy() - lse_ref).max() < 1e-5
    # uniforms inside the reference's drawn intervals: the reference's tuples, exactly
    k = g["idx"]
    lo = np.where(k > 0, cdf[rows, np.maximum(k - 1, 0)], 0.0)
    u = torch.from_numpy((lo + 0.5 * pa[rows, k]).astype(np.float32)).to(DEV)
    la_g, lp_g = la.clone().requires_grad_(True), lp.clone().requires_grad_(True)
    add, conn, term, invalid, like_a, like_p = sampler.sample_actions_rl(la_g, lp_g, n_nodes, edges, dim_f_add,
                                                                         dim_f_conn, uniform=u)
    for j in range(6):
        assert np.array_equal(add[j].cpu().numpy(), g[f"add{j}"]), f"add[{j}]"
    for j in range(4):
        assert np.array_equal(conn[j].cpu().numpy(), g[f"conn{j}"]), f"conn[{j}]"
    assert np.array_equal(term.cpu().numpy(), g["term"])
    assert np.array_equal(invalid.cpu().numpy(), g["invalid"])
    assert np.abs(like_a.detach().cpu().numpy() - g["agent_likelihoods"]).max() < 1e-6
    assert np.abs(like_p.detach().cpu().numpy() - g["prior_likelihoods"]).max() < 1e-6
    assert np.all(like_a.detach().cpu().numpy() > 0) and np.all(like_p.detach().cpu().numpy() > 0)
    ((like_a * torch.from_numpy(g["wa"]).to(DEV)).sum() + (like_p * torch.from_numpy(g["wp"]).to(DEV)).sum()).backward()
    assert np.abs(la_g.grad.cpu().numpy() - g["grad_agent"]).max() < 2e-7
    assert np.abs(lp_g.grad.cpu().numpy() - g["grad_prior"]).max() < 2e-7


def test_rl_sampler_agrees_with_sample_actions_bit_for_bit(golden_dir):
    g, dim_f_add, dim_f_conn, A = _fixture(golden_dir)
    n_nodes = torch.from_numpy(g["n_nodes"]).to(DEV)
    edges = torch.from_numpy(g["edges"]).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    B, W = g["agent_logits"].shape
    for pitch in (W, W + 3):                                      # scalar and float4 loads of the agent row
        la = (torch.randn(B, pitch, device=DEV, generator=gen) * 3)[:, :W]
        lp = torch.randn(B, W, device=DEV, generator=gen)
        u = torch.rand(B, device=DEV, generator=gen)
        a1, l1, f1 = sampler.sample_actions_raw(la, n_nodes, edges, A, uniform=u)
        a2, l2, _, f2, _, _ = sampler.sample_actions_rl_raw(la, lp, n_nodes, edges, A, uniform=u)
        assert torch.equal(a1, a2) and torch.equal(f1, f2) and torch.equal(l1, l2), pitch


def _dims_for(W):
    return {625: (13, 45, 3), 9769: (88, 108, 3), 15360: (1, 15356, 3), 15361: (1, 15357, 3)}[W]


def _autograd_ref(la, lp, idx, wa, wp):
    la64, lp64 = la.detach().double().requires_grad_(True), lp.detach().double().requires_grad_(True)
    i = idx.long()[:, None]
    loss = (torch.softmax(la64, 1).gather(1, i)[:, 0] * wa.double()).sum() + \
        (torch.softmax(lp64, 1).gather(1, i)[:, 0] * wp.double()).sum()
    loss.backward()
    return la64.grad, lp64.grad


@pytest.mark.parametrize("W,pitch", [(625, 625), (625, 632), (9769, 9769), (15360, 15360), (15360, 15363)])
def test_rl_backward_against_torch_autograd(W, pitch):
    N, A, Fe = _dims_for(W)
    B = 64
    gen = torch.Generator(device=DEV).manual_seed(W + pitch)
    base_a = torch.randn(B, pitch, device=DEV, generator=gen) * 2
    base_p = torch.randn(B, pitch, device=DEV, generator=gen) * 2
    la, lp = base_a.requires_grad_(True), base_p.requires_grad_(True)
    xa, xp = la[:, :W], lp[:, :W]                                 # pitch > W: a strided view, ld = pitch
    n_nodes = torch.randint(0, N + 1, (B,), device=DEV, generator=gen).to(torch.int8)
    edges = torch.zeros((B, N, N, Fe), dtype=torch.int8, device=DEV)
    wa, wp = torch.randn(B, device=DEV, generator=gen), torch.randn(B, device=DEV, generator=gen)
    action, like_a, like_p, flags = sampler._SampleRL.apply(xa, xp, n_nodes, edges, A, None, gen)
    ((like_a * wa).sum() + (like_p * wp).sum()).backward()
    idx = torch.from_numpy(_flat_index(action.cpu().numpy(), N, A, Fe)).to(DEV)
    ga, gp = _autograd_ref(xa, xp, idx, wa, wp)
    for got, ref in ((la.grad[:, :W], ga), (lp.grad[:, :W], gp)):
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        assert err < 1e-5, (W, pitch, err)
    if pitch != W:
        assert float(la.grad[:, W:].abs().max()) == 0.0


def test_rl_backward_prior_without_grad_same_tensor_twice_and_none_upstream():
    N, A, Fe = _dims_for(625)
    W, B = 625, 128
    gen = torch.Generator(device=DEV).manual_seed(1)
    n_nodes = torch.randint(0, N + 1, (B,), device=DEV, generator=gen).to(torch.int8)
    edges = torch.zeros((B, N, N, Fe), dtype=torch.float32, device=DEV)
    dims = ([N, 5, 3, 3], [N, Fe])
    u = torch.rand(B, device=DEV, generator=gen)
    wa, wp = torch.randn(B, device=DEV, generator=gen), torch.randn(B, device=DEV, generator=gen)
    la = (torch.randn(B, W, device=DEV, generator=gen) * 2).requires_grad_(True)
    with torch.no_grad():
        lp = torch.randn(B, W, device=DEV, generator=gen) * 2
    # a prior produced under no_grad: the agent side only
    out = sampler.sample_actions_rl(la, lp, n_nodes, edges, *dims, uniform=u)
    assert not out[5].requires_grad and out[4].requires_grad
    (out[4] * wa).sum().backward()
    action = sampler.sample_actions_rl_raw(la, lp, n_nodes, edges, A, u)[0]
    idx = torch.from_numpy(_flat_index(action.cpu().numpy(), N, A, Fe)).to(DEV)
    ga, _ = _autograd_ref(la, lp, idx, wa, torch.zeros_like(wp))
    assert float((la.grad.double() - ga).abs().max() / ga.abs().max()) < 1e-5
    # one tensor as agent and prior: the two gradients add up
    la.grad = None
    out = sampler.sample_actions_rl(la, la, n_nodes, edges, *dims, uniform=u)
    assert torch.allclose(out[4], out[5], rtol=1e-6, atol=0)   # chunked vs online sums: last-bit differences
    ((out[4] * wa).sum() + (out[5] * wp).sum()).backward()
    ga, _ = _autograd_ref(la, la, idx, wa + wp, torch.zeros_like(wp))
    assert float((la.grad.double() - ga).abs().max() / ga.abs().max()) < 1e-5
    # a None upstream gradient for one output: that side is skipped
    la.grad = None
    lp2 = lp.clone().requires_grad_(True)
    out = sampler.sample_actions_rl(la, lp2, n_nodes, edges, *dims, uniform=u)
    (out[5] * wp).sum().backward()
    assert la.grad is None
    _, gp = _autograd_ref(la, lp2, idx, torch.zeros_like(wa), wp)
    assert float((lp2.grad.double() - gp).abs().max() / gp.abs().max()) < 1e-5
    # the row limit
    N1, A1, Fe1 = _dims_for(15361)
    big = torch.zeros(2, 15361, device=DEV)
    with pytest.raises(RuntimeError):
        sampler.sample_actions_rl(big, big, torch.zeros(2, dtype=torch.int8, device=DEV),
                                  torch.zeros((2, N1, N1, Fe1), device=DEV), [N1, A1], [N1, Fe1])


class _KernelDraws:
    """sample_actions_rl with the golden's uniforms, round by round; the fp64 draw on the same logits records how
    close each draw came to a CDF boundary."""

    def __init__(self, seed, B, consts):
        self.ref = CO.InverseCdfDraws(seed, B)
        self.consts = consts

    def __call__(self, agent_logits, prior_logits, n_nodes, edges):
        u = torch.from_numpy(self.ref.u[self.ref.round].astype(np.float32)).to(DEV)
        self.ref(SO.softmax_rows(agent_logits.detach().cpu().numpy()))          # margin bookkeeping only
        return sampler.sample_actions_rl(agent_logits, prior_logits, n_nodes, edges, self.consts.dim_f_add,
                                         self.consts.dim_f_conn, uniform=u)


def test_rl_loop_on_the_dropin_ggnn_matches_the_reference_run(golden_dir):
    from graphinvent_amd.gnn import mpnn
    G = np.load(os.path.join(golden_dir, "golden_generator_rl.npz"))
    Gw = np.load(os.path.join(golden_dir, "golden_generator.npz"))
    cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
    consts = RC.as_constants(dict(RC.constants_dict("cuda", cfg, "/nonexistent", batch_size=int(G["batch"]),
                                                    epochs=1), sigma=float(G["sigma"])))
    B = int(G["batch"])
    agent = mpnn.GGNN(constants=consts)
    agent.load_state_dict({k[3:]: torch.from_numpy(Gw[k]) for k in Gw.files if k.startswith("w::")})
    prior = RL.perturbed_prior(agent)                             # on the host: the golden's exact weights
    assert np.allclose(RL.weight_digest(prior), G["prior_digest"], rtol=1e-6, atol=1e-6)
    agent, prior = agent.to(DEV).train(), prior.to(DEV).eval()
    draws = _KernelDraws(int(G["draw_seed"]), B, consts)
    gen = RL.GeneratorRLOracle(agent, prior, B, consts, sampler=draws)
    n = gen.build_graphs()
    assert (n, gen.rounds, draws.ref.round) == (int(G["n_generated"]), int(G["rounds"]), int(G["rounds"]))
    assert draws.ref.margin > 1e-5
    assert np.array_equal(gen.generated_n_nodes.cpu().numpy(), G["n_nodes"])
    assert np.array_equal(gen.generated_nodes.cpu().numpy().astype(np.int8), G["nodes"])
    assert np.array_equal(gen.generated_edges.cpu().numpy().astype(np.int8), G["edges"])
    assert np.array_equal(gen.properly_terminated.cpu().numpy(), G["terminated"])
    a_ll, p_ll = gen.loglikelihoods()
    assert np.allclose(a_ll.detach().cpu().numpy(), G["agent_ll"], rtol=1e-4, atol=0)
    assert np.allclose(p_ll.detach().cpu().numpy(), G["prior_ll"], rtol=1e-4, atol=0)
    loss = torch.mean(RL.compute_loss_component(torch.from_numpy(G["scores"]).to(DEV), a_ll, p_ll,
                                                torch.from_numpy(G["uniqueness"]).to(DEV), float(G["sigma"])))
    loss.backward()
    for model, prefix in ((agent, "ga::"), (prior, "gp::")):
        l2, worst = RL.grad_errors(model, G, prefix)
        print(f"\n[{prefix}] drop-in GGNN + sample_actions_rl vs the reference run: global L2 {l2:.2e}, "
              f"worst tensor {worst:.2e}, loss {float(loss.detach()):.6f} (reference {float(G['loss']):.6f})")
        assert l2 <= 5e-3 and worst <= 3e-2, (prefix, l2, worst)
