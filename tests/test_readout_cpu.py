"""The reference of tests/test_readout_gpu.py checked without a GPU: the hand-written backward formulas of
tests/readout_model.py against torch autograd of the forward expression in fp64 (the last four lines of
``oracle.ggnn_oracle.graph_gather``), expand / compress as transposes of each other, and ``adam_reference`` against
``torch.optim.Adam``."""
import pytest
import torch

from tests import readout_model as RM

BIG = 1e6
TOL = 1e-12


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def _case(N, G, spread=3.0, seed=0):
    cidx, mask, S = RM.batch_layout(N)
    g = torch.Generator().manual_seed(1000 * N + G + seed)
    en = spread * torch.randn(S + 1, G, generator=g)
    emb = torch.randn(S + 1, G, generator=g)
    dgs = [torch.randn(cidx.shape[0], G, generator=g) for _ in range(3)]
    return cidx, mask, S, en, emb, dgs


def test_batch_layout_has_the_masking_cases():
    for N in (1, 5, 13, 128):
        cidx, mask, S = RM.batch_layout(N)
        B = cidx.shape[0]
        assert B == (5 if N >= 4 else 4)
        pad = cidx == S
        assert int((~pad[0]).sum()) == 1 and not bool(pad[0, 0])
        assert not bool(pad[1].any()) and bool((mask[1] == 1).all())
        assert int((~pad[2]).sum()) == 1 and not bool(pad[2, N // 2])
        assert int((~pad[3]).sum()) == 1 and int(mask[3].sum()) == 0           # every slot of graph 3 is masked
        assert bool((mask[pad] == 0).all())
        if N >= 4:
            assert int((~pad[4]).sum()) == N // 2 and int(mask[4].sum()) == N // 2 - 1
    with pytest.raises(AssertionError):
        RM.check_layout(torch.tensor([[0, 0, 2]]), 2)                          # row 0 twice, row 1 never
    with pytest.raises(AssertionError):
        RM.check_layout(torch.tensor([[0, 3]]), 1)                             # past the zero row


@pytest.mark.parametrize("spread", [3.0, 100.0])
@pytest.mark.parametrize("N,G", [(1, 4), (5, 7), (13, 9), (128, 3)])
def test_gather_backward_is_autograd_of_the_forward_expression(N, G, spread):
    """Per graph b: the gradient of sum(out[b] * dg[b]) with respect to the energies and embeddings.  Rows < S receive
    de / dm of their one slot (a factor plane of ones stands for the activation), row S the zero-row partial sums of
    graph b.  The energies enter with the reference's masked value fl32(en[cidx] - penalty) and the gradient path of
    ``energies = raw - energy_mask``."""
    cidx, mask, S, en, emb, dgs = _case(N, G, spread)
    c = cidx.long()
    B = c.shape[0]
    dg = dgs[0].double() + dgs[1].double() + dgs[2].double()
    ones = torch.ones(S + 1, G, dtype=torch.float64)
    en_new, emb_new, zpart = RM.gather_backward(en, emb, cidx, mask, BIG, S, dgs, ones, ones)
    assert torch.equal(en_new[S], en[S].double()) and torch.equal(emb_new[S], emb[S].double())
    q_ref = RM.masked_energies(en, cidx, mask, BIG)
    e64 = en.double().requires_grad_(True)
    m64 = emb.double().requires_grad_(True)
    q = q_ref + (e64[c] - e64[c].detach())                 # the value of q_ref exactly, the gradient path of e64[c]
    attention = torch.softmax(q, dim=1)
    out = torch.sum(attention * m64[c], dim=1)
    assert rel(RM.gather_forward(en, emb, cidx, mask, BIG), out.detach()) < TOL
    d_en, d_emb = torch.zeros(S, G, dtype=torch.float64), torch.zeros(S, G, dtype=torch.float64)
    for b in range(B):
        ge, gm = torch.autograd.grad((out[b] * dg[b]).sum(), (e64, m64), retain_graph=True)
        d_en += ge[:S]; d_emb += gm[:S]
        scale = max(float(ge.abs().max()), float(gm.abs().max()), 1e-300)
        assert float((zpart[b, :G] - ge[S]).abs().max()) <= TOL * scale
        assert float((zpart[b, G:] - gm[S]).abs().max()) <= TOL * scale
        if not bool((c[b] == S).any()):
            assert bool((zpart[b] == 0).all())
    assert float((en_new[:S] - d_en).abs().max()) <= TOL * max(float(d_en.abs().max()), float(dg.abs().max()))
    assert rel(emb_new[:S], d_emb) < TOL


def test_gather_backward_applies_selu_grad_or_the_factor_plane():
    cidx, mask, S, en, emb, dgs = _case(5, 6)
    ones = torch.ones(S + 1, 6, dtype=torch.float64)
    raw_en, raw_emb, z0 = RM.gather_backward(en, emb, cidx, mask, BIG, S, dgs[0], ones, ones)
    act_en, act_emb, z1 = RM.gather_backward(en, emb, cidx, mask, BIG, S, dgs[0])
    assert torch.equal(z0, z1)                                                  # the partial sums carry no factor
    assert rel(act_en[:S], raw_en[:S] * RM.selu_grad_from_out(en[:S])) < TOL
    assert rel(act_emb[:S], raw_emb[:S] * RM.selu_grad_from_out(emb[:S])) < TOL
    y = torch.tensor([-1.5, 0.0, 2.0])
    expect = torch.tensor([-1.5 + RM.SELU_SCALE * RM.SELU_ALPHA, RM.SELU_SCALE * RM.SELU_ALPHA, RM.SELU_SCALE],
                          dtype=torch.float64)
    assert torch.equal(RM.selu_grad_from_out(y), expect)
    z = torch.linspace(-3, 3, 61, dtype=torch.float64).requires_grad_(True)     # and it is selu' indeed
    s = torch.selu(z)
    assert rel(RM.selu_grad_from_out(s.detach()), torch.autograd.grad(s.sum(), z)[0]) < TOL
    g = torch.Generator().manual_seed(3)
    fe, fm = 2 * torch.rand(S + 1, 6, generator=g), 2 * torch.rand(S + 1, 6, generator=g)
    f_en, f_emb, _ = RM.gather_backward(en, emb, cidx, mask, BIG, S, dgs[0], fe, fm)
    assert rel(f_en[:S], raw_en[:S] * fe[:S].double()) < TOL and rel(f_emb[:S], raw_emb[:S] * fm[:S].double()) < TOL


@pytest.mark.parametrize("N,W", [(1, 5), (13, 3), (128, 2)])
def test_expand_and_compress_are_transposes(N, W):
    cidx, mask, S = RM.batch_layout(N)
    B = cidx.shape[0]
    g = torch.Generator().manual_seed(N + W)
    t1 = torch.randn(S + 1, W, generator=g, dtype=torch.float64).requires_grad_(True)
    dcat = torch.randn(B, N * W, generator=g, dtype=torch.float64)
    cat = RM.expand(t1, cidx)
    assert cat.shape == (B, N * W)
    assert all(torch.equal(cat[b, n * W:(n + 1) * W], t1[int(cidx[b, n])]) for b in range(B) for n in range(N))
    grad = torch.autograd.grad((cat * dcat).sum(), t1)[0]
    new, zpart = RM.compress(t1.detach(), cidx, S, dcat, torch.ones(S + 1, W, dtype=torch.float64))
    assert rel(new[:S], grad[:S]) < TOL and torch.equal(new[S], t1.detach()[S])
    assert float((zpart.sum(0) - grad[S]).abs().max()) <= TOL * max(float(grad.abs().max()), 1.0)
    for b in range(B):                                     # per graph: the slots on the zero row, summed
        pad = (cidx[b] == S).double()
        assert rel(zpart[b], (dcat[b].reshape(N, W) * pad.unsqueeze(-1)).sum(0)) < TOL or not bool(pad.any())
        if not bool(pad.any()):
            assert bool((zpart[b] == 0).all())
    act, _ = RM.compress(t1.detach(), cidx, S, dcat)
    assert rel(act[:S], grad[:S] * RM.selu_grad_from_out(t1.detach()[:S])) < TOL


def test_gradient_sums_against_loops():
    g = torch.Generator().manual_seed(9)
    part = torch.randn(17, 5, generator=g)
    y = torch.tensor([-1.0, 0.0, 0.5, -0.2, 3.0])
    want = torch.stack([sum(part[r, c].double() for r in range(17)) for c in range(5)])
    assert rel(RM.colsum(part), want) < TOL
    assert rel(RM.colsum(part, y), want * RM.selu_grad_from_out(y)) < TOL
    assert RM.colsum(part[:0]).shape == (5,) and bool((RM.colsum(part[:0], y) == 0).all())
    slabs = torch.randn(3, 4, 5, generator=g)
    yy = torch.randn(4, 5, generator=g)
    want = (slabs[0].double() + slabs[1].double() + slabs[2].double()) * RM.selu_grad_from_out(yy)
    assert rel(RM.slab_sum_dselu(slabs, yy), want) < TOL
    dW, db = RM.reduce_slabs(slabs)
    assert dW.shape == (4, 4) and db.shape == (4,)
    assert rel(dW, slabs.double().sum(0)[:, :4]) < TOL and rel(db, slabs.double().sum(0)[:, 4]) < TOL


def test_adam_reference_is_torch_adam_when_nothing_skips():
    g = torch.Generator().manual_seed(21)
    shapes = [(7, 5), (3,), (1,), (64, 9), (2, 2)]
    init = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
    groups = [dict(idx=[0, 1, 2], lr=3e-3, weight_decay=1e-2), dict(idx=[3, 4], lr=1e-3, weight_decay=0.0)]
    grads = [[torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes] for _ in range(8)]
    history = RM.adam_reference(init, groups, grads)
    ps = [torch.nn.Parameter(x.clone()) for x in init]
    opt = torch.optim.Adam([dict(params=[ps[i] for i in grp["idx"]], lr=grp["lr"], weight_decay=grp["weight_decay"])
                            for grp in groups])
    for step_grads, (p_ref, m_ref, v_ref) in zip(grads, history):
        for p, gr in zip(ps, step_grads):
            p.grad = gr.clone()
        opt.step()
        for i, p in enumerate(ps):
            assert rel(p_ref[i], p.detach()) < TOL
            assert rel(m_ref[i], opt.state[p]["exp_avg"]) < TOL and rel(v_ref[i], opt.state[p]["exp_avg_sq"]) < TOL


def test_adam_reference_skips_a_parameter_without_a_gradient():
    """Nothing of a skipped parameter moves; the group's count goes on, so the next step is corrected with it."""
    init = [torch.tensor([1.0, -2.0]), torch.tensor([0.5])]
    groups = [dict(idx=[0, 1], lr=0.1, weight_decay=0.1)]
    g0, g1 = torch.tensor([0.3, 0.4]), torch.tensor([-0.7])
    history = RM.adam_reference(init, groups, [[g0, g1], [g0, None], [g0, g1]])
    for k in range(3):
        assert torch.equal(history[0][k][1], history[1][k][1])
    lone = RM.adam_reference(init, groups, [[g0, g1], [g0, g1]])
    assert not torch.equal(history[2][0][1], lone[1][0][1])                     # corrected with count 3, not 2
    g = g1.double() + 0.1 * history[1][0][1]
    m = history[1][1][1] + 0.1 * (g - history[1][1][1])
    v = 0.999 * history[1][2][1] + 0.001 * g * g
    want = history[1][0][1] - 0.1 / (1 - 0.9 ** 3) * (m / (v.sqrt() / (1 - 0.999 ** 3) ** 0.5 + 1e-8))
    assert rel(history[2][0][1], want) < TOL
