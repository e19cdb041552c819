"""Test helper: the plain torch specification of the segmented reductions of csrc/gi_ops.hip (gi_seg_sum, gi_seg_sum_dselu[_f],
gi_class_sum_dselu, gi_seg_softmax_fwd / _bwd), of the SELU-backward row kernels (gi_selu_bwd_rows_f, gi_selu_bwd_cols3_f)
and of gi_slab_epilogue.  Written from the comments of include/graphinvent_amd.h, not from the kernels, and importing
nothing of the package.  Every function takes ``dtype``: float64 is the reference, float32 the same formulas in the
kernels' own precision — the yardstick a kernel's error is measured with (tests/test_segments_gpu.py).

A CSR is (perm [E] int32, off [rows + 1] int32): segment c holds the slots off[c] .. off[c + 1] - 1, slot k reads value
row perm[k].  Functions take buffers cut to their payload columns.

  seg_sum          out[c] = (base[c] +) sum_k vals[perm[k]]
  seg_sum_dact     y[c] <- dact[c] * sum_k vals[perm[k]];  dact = selu' through the stored output y, or ``factor``
  class_sum_dact   the same function (gi_class_sum_dselu differs in its launch shape only)
  seg_softmax      att[k] = softmax over the slots of a segment of en[perm[k]];  agg[c] = sum_k att[k] * emb[perm[k]]
                   (an empty segment: agg = 0)
  seg_softmax_bwd  d_emb_e[k] = att[k] * dagg[c];  d_en_e[k] = att[k] * (emb[perm[k]] * dagg[c] - <att, emb * dagg>_c)
  dact_rows        out[r] = dY[idx[r]] * dact[r]   (idx None: dY[r])
  slab_epilogue    x = sum_s slabs[s]; + bias; selu; * selu'(act) or * act; + base — by the GI_EPI_* flags
  csr              the CSR of a list of segment lengths over V value rows"""
import torch

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946
F64, F32 = torch.float64, torch.float32
EPI_BIAS, EPI_SELU, EPI_DSELU, EPI_ACCUM, EPI_MULACT = 1, 2, 4, 8, 64        # GI_EPI_* of include/graphinvent_amd.h


def selu(x, dtype=F64):
    """scale * (x > 0 ? x : alpha * (exp(x) - 1))"""
    x = x.to(dtype)
    neg = torch.tensor(SELU_ALPHA, dtype=dtype) * (torch.exp(torch.clamp(x, max=0.0)) - 1.0)
    return torch.tensor(SELU_SCALE, dtype=dtype) * torch.where(x > 0, x, neg)


def selu_grad_from_out(y, dtype=F64):
    """selu' from the stored output y = selu(z): scale for y > 0, else y + scale * alpha."""
    y = y.to(dtype)
    return torch.where(y > 0, torch.full_like(y, SELU_SCALE), y + torch.tensor(SELU_SCALE * SELU_ALPHA, dtype=dtype))


def csr(lengths, V, seed=0, repeat_in=None):
    """(perm, off) int32 of segments with the given lengths, in the given order.  off is their running sum; the slots
    of a segment read distinct rows drawn from the V value rows with a seeded generator (a segment longer than V draws
    with replacement).  repeat_in = c: segment c (length >= 2) reads the row of its first slot in its second slot too."""
    lengths = [int(n) for n in lengths]
    assert V >= 1 and all(n >= 0 for n in lengths)
    g = torch.Generator().manual_seed(seed)
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.tensor(lengths, dtype=torch.int64).cumsum(0) if lengths else 0
    parts = [torch.randperm(V, generator=g)[:n] if n <= V else torch.randint(0, V, (n,), generator=g) for n in lengths]
    perm = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)
    if repeat_in is not None:
        assert lengths[repeat_in] >= 2
        perm[off[repeat_in] + 1] = perm[off[repeat_in]]
    return perm.to(torch.int32), off.to(torch.int32)


def seg_lengths(off):
    off = off.long()
    return off[1:] - off[:-1]


def slot_segments(off):
    """[E] the segment of every slot."""
    n = seg_lengths(off)
    return torch.repeat_interleave(torch.arange(n.numel()), n)


def _slot_sum(x, off, rows):
    """[rows, cols]: the per-segment sums of the slot-ordered rows x [E, cols], added in slot order."""
    out = torch.zeros(rows, x.shape[1], dtype=x.dtype)
    if x.shape[0]:
        out.index_add_(0, slot_segments(off)[:x.shape[0]], x)
    return out


def seg_sum(vals, perm, off, rows, base=None, dtype=F64):
    off = off[:rows + 1]
    E = int(off[rows])
    s = _slot_sum(vals.to(dtype)[perm[:E].long()], off, rows)
    return s if base is None else s + base.to(dtype)


def seg_sum_dact(vals, perm, off, y, factor=None, dtype=F64):
    """y [rows, cols] the stored outputs; factor [rows, cols] replaces selu'(y) when given."""
    f = selu_grad_from_out(y, dtype) if factor is None else factor.to(dtype)
    return seg_sum(vals, perm, off, y.shape[0], dtype=dtype) * f


class_sum_dact = seg_sum_dact


def _attention(en, perm, off, dtype):
    """[E, cols]: the softmax of every segment, by hand: max, exp of the difference, sum, quotient."""
    rows = off.numel() - 1
    seg = slot_segments(off)
    q = en.to(dtype)[perm.long()]
    idx = seg.unsqueeze(1).expand_as(q)
    mx = torch.zeros(rows, q.shape[1], dtype=dtype).scatter_reduce_(0, idx, q, "amax", include_self=False)
    e = torch.exp(q - mx[seg])
    return e / _slot_sum(e, off, rows)[seg]


def seg_softmax(en, emb, perm, off, dtype=F64):
    """(agg [rows, cols], att [E, cols])"""
    att = _attention(en, perm, off, dtype)
    return _slot_sum(att * emb.to(dtype)[perm.long()], off, off.numel() - 1), att


def seg_softmax_bwd(dagg, en, emb, perm, off, dtype=F64):
    """(d_en_e, d_emb_e), [E, cols] each, in slot order."""
    rows = off.numel() - 1
    seg = slot_segments(off)
    att = _attention(en, perm, off, dtype)
    d = dagg.to(dtype)[seg]
    ed = emb.to(dtype)[perm.long()] * d
    inner = _slot_sum(att * ed, off, rows)
    return att * (ed - inner[seg]), att * d


def dact_rows(dY, idx, Y, factor=None, dtype=F64):
    """out [rows, cols]; dY [*, cols], idx [rows] or None, Y [rows, cols] the stored outputs."""
    src = dY.to(dtype) if idx is None else dY.to(dtype)[idx.long()]
    return src * (selu_grad_from_out(Y, dtype) if factor is None else factor.to(dtype))


def slab_epilogue(slabs, flags, bias=None, act=None, base=None, dtype=F64):
    """slabs [nsplit, rows, cols]; bias [cols]; act / base [rows, cols]."""
    x = slabs.to(dtype).sum(dim=0)
    if flags & EPI_BIAS:
        x = x + bias.to(dtype)
    if flags & EPI_SELU:
        x = selu(x, dtype)
    if flags & EPI_DSELU:
        x = x * selu_grad_from_out(act, dtype)
    if flags & EPI_MULACT:
        x = x * act.to(dtype)
    if flags & EPI_ACCUM:
        x = x + base.to(dtype)
    return x
