"""The reference of tests/test_segments_gpu.py checked without a GPU: tests/segment_model.py against torch.softmax per
segment, against Python loops, and — the hand-written backward formulas — against torch autograd of the forward
expressions in fp64."""
import pytest
import torch

from tests import segment_model as SM

TOL = 1e-12
F64 = torch.float64
LENGTHS = [0, 0, 1, 2, 3, 7, 0, 40, 5, 2, 0]


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def _energies(kind, V, cols, g):
    if kind == "randn":
        return 3 * torch.randn(V, cols, generator=g)
    return (2 * torch.rand(V, cols, generator=g) - 1) * 100


def test_csr_builder():
    lengths = [0, 3, 0, 0, 1, 300, 2, 0]
    perm, off = SM.csr(lengths, 64, seed=5)
    assert perm.dtype == torch.int32 and off.dtype == torch.int32
    assert int(off[0]) == 0 and off.numel() == len(lengths) + 1 and perm.numel() == sum(lengths) == int(off[-1])
    assert bool((off[1:] >= off[:-1]).all())
    assert SM.seg_lengths(off).tolist() == lengths                            # the requested lengths, in order
    assert int(perm.min()) >= 0 and int(perm.max()) < 64
    assert SM.slot_segments(off).tolist() == [1] * 3 + [4] + [5] * 300 + [6] * 2
    for c, n in enumerate(lengths):                                          # distinct rows wherever they fit
        seg = perm[int(off[c]):int(off[c + 1])]
        assert n > 64 or seg.unique().numel() == n
    again, _ = SM.csr(lengths, 64, seed=5)
    other, _ = SM.csr(lengths, 64, seed=6)
    assert torch.equal(perm, again) and not torch.equal(perm, other)
    rep, off2 = SM.csr(lengths, 64, seed=5, repeat_in=1)
    assert torch.equal(off2, off) and int(rep[0]) == int(rep[1]) == int(perm[0])
    assert torch.equal(rep[2:], perm[2:])
    with pytest.raises(AssertionError):
        SM.csr(lengths, 64, repeat_in=4)                                     # a segment of one slot cannot repeat a row
    perm0, off0 = SM.csr([0, 0, 0], 1)
    assert perm0.numel() == 0 and off0.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("cols", [1, 5])
def test_seg_sum_against_a_loop(cols):
    g = torch.Generator().manual_seed(1)
    V = 50
    perm, off = SM.csr(LENGTHS, V, seed=2, repeat_in=5)
    rows = len(LENGTHS)
    vals = torch.randn(V, cols, generator=g)
    base = torch.randn(rows, cols, generator=g)
    want = torch.zeros(rows, cols, dtype=F64)
    for c in range(rows):
        for k in range(int(off[c]), int(off[c + 1])):
            want[c] += vals[int(perm[k])].double()
    assert rel(SM.seg_sum(vals, perm, off, rows), want) < TOL
    assert rel(SM.seg_sum(vals, perm, off, rows, base=base), want + base.double()) < TOL
    assert rel(SM.seg_sum(vals, perm, off, 4), want[:4]) < TOL                 # a CSR cut to its first rows
    assert SM.seg_sum(vals, perm, off, rows, dtype=torch.float32).dtype == torch.float32
    empty = [c for c, n in enumerate(LENGTHS) if n == 0]
    assert bool((SM.seg_sum(vals, perm, off, rows)[empty] == 0).all())


@pytest.mark.parametrize("kind", ["randn", "pm100"])
def test_seg_softmax_against_torch_softmax(kind):
    g = torch.Generator().manual_seed(3)
    V, cols = 60, 7
    perm, off = SM.csr(LENGTHS, V, seed=4, repeat_in=5)
    en, emb = _energies(kind, V, cols, g), torch.randn(V, cols, generator=g)
    agg, att = SM.seg_softmax(en, emb, perm, off)
    assert bool(torch.isfinite(agg).all()) and bool(torch.isfinite(att).all())
    if kind == "pm100":                                                      # ... where exp of the raw energies is not
        assert not bool(torch.isfinite(torch.exp(en) / torch.exp(en)).all())
        a32, t32 = SM.seg_softmax(en, emb, perm, off, dtype=torch.float32)
        assert bool(torch.isfinite(a32).all()) and bool(torch.isfinite(t32).all())
    for c, n in enumerate(LENGTHS):
        lo, hi = int(off[c]), int(off[c + 1])
        if n == 0:
            assert bool((agg[c] == 0).all())
            continue
        p = perm[lo:hi].long()
        want = torch.softmax(en[p].double(), dim=0)
        assert rel(att[lo:hi], want) < TOL
        assert rel(agg[c], (want * emb[p].double()).sum(0)) < TOL


@pytest.mark.parametrize("kind", ["randn", "pm100"])
def test_seg_softmax_bwd_is_autograd_of_the_forward(kind):
    """Per edge slot: the gradient of sum(agg * dagg) with respect to the slot's own copy of its energy and embedding
    row (a row read by two slots receives the sum of both, which is the kernels' next step, not this one)."""
    g = torch.Generator().manual_seed(5)
    V, cols = 60, 4
    perm, off = SM.csr(LENGTHS, V, seed=6, repeat_in=7)
    rows = len(LENGTHS)
    en, emb = _energies(kind, V, cols, g), torch.randn(V, cols, generator=g)
    dagg = torch.randn(rows, cols, generator=g)
    en_e = en.double()[perm.long()].requires_grad_()
    emb_e = emb.double()[perm.long()].requires_grad_()
    loss = torch.zeros((), dtype=F64)
    for c in range(rows):
        lo, hi = int(off[c]), int(off[c + 1])
        if hi > lo:
            loss = loss + ((torch.softmax(en_e[lo:hi], dim=0) * emb_e[lo:hi]).sum(0) * dagg[c].double()).sum()
    loss.backward()
    d_en, d_emb = SM.seg_softmax_bwd(dagg, en, emb, perm, off)
    assert rel(d_en, en_e.grad) < TOL and rel(d_emb, emb_e.grad) < TOL
    seg_sums = torch.zeros(rows, cols, dtype=F64).index_add_(0, SM.slot_segments(off), d_en)
    assert float(seg_sums.abs().max()) < TOL * float(d_en.abs().max())        # the softmax identity


def _stored(shape, g):
    z = 2 * torch.randn(shape, generator=g, dtype=F64)
    z.view(-1)[::5] = 0.0
    return z


@pytest.mark.parametrize("with_factor", [False, True])
def test_seg_sum_dact_is_autograd_of_the_gather(with_factor):
    """Forward: message row u = act(z[u]) is read by every slot k of its segment and lands on edge row perm[k]; the
    loss weighs the edge rows with vals.  act = selu, or the multiplication with a fixed factor."""
    g = torch.Generator().manual_seed(7)
    V, cols = 50, 3
    perm, off = SM.csr(LENGTHS, V, seed=8)
    rows = len(LENGTHS)
    vals = torch.randn(V, cols, generator=g)
    factor = 2 * torch.rand(rows, cols, generator=g) * (torch.rand(rows, cols, generator=g) >= 0.25)
    z = _stored((rows, cols), g).requires_grad_()
    y = z * factor.double() if with_factor else torch.selu(z)
    edge = torch.zeros(V, cols, dtype=F64).index_add(0, perm.long(), y[SM.slot_segments(off)])
    (edge * vals.double()).sum().backward()
    got = SM.seg_sum_dact(vals, perm, off, y.detach(), factor if with_factor else None)
    assert rel(got, z.grad) < TOL
    assert SM.class_sum_dact is SM.seg_sum_dact


@pytest.mark.parametrize("with_factor", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_dact_rows_is_autograd(gather, with_factor):
    g = torch.Generator().manual_seed(9)
    rows, cols, src = 9, 5, 6
    idx = torch.randint(0, src, (rows,), generator=g).int() if gather else None
    dY = torch.randn(src if gather else rows, cols, generator=g)
    factor = 2 * torch.rand(rows, cols, generator=g) * (torch.rand(rows, cols, generator=g) >= 0.25)
    z = _stored((rows, cols), g).requires_grad_()
    y = z * factor.double() if with_factor else torch.selu(z)
    out = torch.zeros(dY.shape, dtype=F64).index_add(0, idx.long(), y) if gather else y
    (out * dY.double()).sum().backward()
    assert rel(SM.dact_rows(dY, idx, y.detach(), factor if with_factor else None), z.grad) < TOL


def test_selu_and_slab_epilogue():
    g = torch.Generator().manual_seed(11)
    x = 3 * torch.randn(200, generator=g, dtype=F64)
    x[::7] = 0.0
    assert rel(SM.selu(x), torch.selu(x)) < TOL
    xs = x.clone().requires_grad_()
    torch.selu(xs).sum().backward()
    assert rel(SM.selu_grad_from_out(torch.selu(x)), xs.grad) < TOL
    nsplit, rows, cols = 3, 4, 5
    slabs = torch.randn(nsplit, rows, cols, generator=g)
    bias, act, base = torch.randn(cols, generator=g), torch.selu(torch.randn(rows, cols, generator=g)), \
        torch.randn(rows, cols, generator=g)
    s = slabs.double()[0] + slabs.double()[1] + slabs.double()[2]
    assert rel(SM.slab_epilogue(slabs, 0), s) < TOL
    assert rel(SM.slab_epilogue(slabs, SM.EPI_BIAS | SM.EPI_SELU, bias=bias), torch.selu(s + bias.double())) < TOL
    assert rel(SM.slab_epilogue(slabs, SM.EPI_DSELU | SM.EPI_ACCUM, act=act, base=base),
               s * SM.selu_grad_from_out(act) + base.double()) < TOL
    assert rel(SM.slab_epilogue(slabs, SM.EPI_MULACT, act=act), s * act.double()) < TOL
