"""-m gpu: the segmented reductions of csrc/gi_ops.hip (gi_seg_sum in both instantiations, gi_seg_sum_dselu[_f],
gi_class_sum_dselu, gi_seg_softmax_fwd / _bwd), gi_selu_bwd_rows_f / gi_selu_bwd_cols3_f and gi_slab_epilogue against an
independent reference (tests/segment_model.py in fp64), called through the C ABI at the segment lengths, column counts
and thread counts where the kernels change path.

Copies, untouched memory and "exactly 0" are compared as bits (outputs start as 7.0; what lies beyond r4(cols), and what a
kernel is documented not to touch, must still be 7.0 afterwards).  Everything else follows the rule of
tests/test_readout_gpu.py — the error against fp64 must stay within 8 x the error of the same formulas run in fp32 on
the CPU for the same case, floor 1e-6; the 8 is that file's: serial against pairwise sums (x 4) and a different expf
(x 2) — with one difference: the error is taken PER SEGMENT-LENGTH CLASS.  Rows are grouped by the length of their
segment (the per-edge rows of the softmax backward by the length of the segment they belong to) and each group is held
to its own scale, err = max|got - ref64| / max|ref64| over the group: over the whole tensor the long segments set the
scale and an error in the rows of length 1 or 3 is invisible.  A group whose reference is all zero (empty segments)
must be zero.  Summed values carry one sign per column, so no sum cancels and a group's scale also bounds each of its
outputs.  The one output that is a difference by its formula, d_en_e = att * emb * dagg - att * <att, emb * dagg>,
takes as its scale the larger of max|ref64| and the fp64 size of these two terms over the group's edges: both carry the
fp32 rounding of a number of that size, whatever is left of their difference — nothing in a one-edge segment (where a
contracted multiply-subtract leaves the rounding residue of emb * dagg) and less than one ulp of the terms in a
saturated softmax (energies 100 apart: the true gradient is of the order exp(-100), the fp32 formulas are 100 % off
and measure nothing).  Every figure is printed before it is asserted (pytest -s); the lines
"share <kernel> <error / bound>" are what docs/MEASUREMENTS_LOG.md records."""
import functools
import types

import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import ops
from tests import segment_model as SM

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAINT = 7.0
EINVAL = -1
F32, F64 = torch.float32, torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def painted(t):
    return bool((t == PAINT).all())


def zero_bits(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def held(kernel, name, got, ref64, ref32, cls=None, operands=None):
    """The tolerance of this file (module docstring).  cls: the class of every row of got (None: one class);
    operands: per row the size of the numbers whose difference the row is."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape)
    n = got.shape[0]
    if n == 0:
        return
    cls = torch.zeros(n, dtype=torch.long) if cls is None else cls.long()
    assert cls.numel() == n
    err_r = torch.nan_to_num((got - ref64).abs().reshape(n, -1).amax(dim=1), nan=float("inf"))
    ref_r = ref64.abs().reshape(n, -1).amax(dim=1)
    yard_r = (ref32.double() - ref64).abs().reshape(n, -1).amax(dim=1)
    for k in sorted(set(cls.tolist())):
        m = cls == k
        scale = float(ref_r[m].max())
        if operands is not None:
            scale = max(scale, float(operands[m].max()))
        if scale == 0.0:
            worst = float(torch.nan_to_num(got[m].abs(), nan=float("inf")).max())
            print(f"{name} class {k}: reference all zero, kernel max {worst:.3e}")
            assert worst == 0.0, (name, k)
            continue
        e = float(err_r[m].max()) / scale
        yard = float(yard_r[m].max()) / scale
        bound = max(8.0 * yard, 1e-6)
        print(f"{name} class {k}: kernel {e:.3e} yardstick {yard:.3e} bound {bound:.3e} (scale {scale:.3e})")
        print(f"share {kernel} {e / bound:.4f}")
        assert e <= bound, (name, k)


def padded(t, ld, rows=None):
    """[rows, ld] on the device, painted, with t in its first columns."""
    buf = torch.full((t.shape[0] if rows is None else rows, ld), PAINT, dtype=F32)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.to(DEV)


def with_plane(t, f, ld):
    """[2, rows, ld]: the activations, and the factor plane fshift = rows * ld floats behind them."""
    assert (t.shape[0] * ld) % 4 == 0
    return torch.stack((padded(t, ld), padded(f, ld)))


def factors(shape, g):
    """AlphaDropout factors: random in [0, 2), about a quarter exactly 0 (dropped units)."""
    return 2 * torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) >= 0.25)


def stored_outputs(shape, g):
    """SELU outputs of both signs (> -scale * alpha) with exact zeros among them."""
    y = torch.selu(2 * torch.randn(shape, generator=g))
    y.view(-1)[::3] = 0.0
    return y


def column_signs(cols, g):
    return (torch.randint(0, 2, (1, cols), generator=g) * 2 - 1).float()


def magnitudes(shape, g):
    return torch.rand(shape, generator=g) + 0.5


# ---- 1. gi_seg_sum, one output per thread ----------------------------------------------------------------------------
# every length of {0, 1, 2, 3, 4, 5, 6, 7, 9, 33, 300}: none / one row of the first pair, the pair, the odd tail after it,
# one, two and more turns of the pair loop with and without a tail; empty segments first, last and adjacent
SEG_LENGTHS = [0, 0, 1, 2, 3, 0, 4, 5, 6, 7, 9, 33, 300, 1, 3, 2, 5, 0]
SEG_V = 64


def cycled(lengths, n):
    return [lengths[i % len(lengths)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _sum_case(n_rows, cols, seed=0):
    """Values, CSR, accumulate base, stored outputs and factors of n_rows segments, with the references of seg_sum
    (plain, accumulate) and seg_sum_dact (selu', factor); computed once and never written."""
    g = torch.Generator().manual_seed(9000 + 7 * n_rows + cols + seed)
    c = types.SimpleNamespace(rows=n_rows, cols=cols)
    lengths = cycled(SEG_LENGTHS, n_rows) if n_rows != 1 else [5]
    c.perm, c.off = SM.csr(lengths, SEG_V, seed=n_rows + cols)
    c.cls = SM.seg_lengths(c.off)
    sign = column_signs(cols, g)
    c.vals = magnitudes((SEG_V, cols), g) * sign
    c.base = magnitudes((n_rows, cols), g) * sign
    c.y = stored_outputs((n_rows, cols), g)
    c.f = factors((n_rows, cols), g)
    c.sum = {(acc, dt): SM.seg_sum(c.vals, c.perm, c.off, n_rows, base=c.base if acc else None, dtype=dt)
             for acc in (0, 1) for dt in (F64, F32)}
    c.dact = {(plane, dt): SM.seg_sum_dact(c.vals, c.perm, c.off, c.y, c.f if plane else None, dtype=dt)
              for plane in (False, True) for dt in (F64, F32)}
    c.perm_d, c.off_d = c.perm.to(DEV), c.off.to(DEV)
    return c


def _run_seg_sum(c, accumulate, tag):
    lib = L.load()
    rows, cols = c.rows, c.cols
    r4 = ops.r4(cols)
    ldv, ldo = r4 + 4, r4 + 8
    vals = padded(c.vals, ldv)
    vals_in = vals.clone()
    out = torch.full((rows + 1, ldo), PAINT, device=DEV)
    if accumulate:
        out[:rows, :cols] = c.base.to(DEV)
    L.check(lib.gi_seg_sum(vals.data_ptr(), ldv, c.perm_d.data_ptr(), c.off_d.data_ptr(), rows, cols, out.data_ptr(),
                           ldo, accumulate, _stream()), "seg_sum")
    held("seg_sum<1>", tag, out[:rows, :cols], c.sum[accumulate, F64], c.sum[accumulate, F32], c.cls)
    assert painted(out[:, r4:]) and painted(out[rows]) and same_bits(vals, vals_in)
    empty = (c.cls == 0).nonzero().flatten().to(DEV)
    if empty.numel():
        if accumulate:
            assert same_bits(out[empty, :cols], c.base[empty.cpu()])
        else:
            assert zero_bits(out[empty, :cols])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cols", [1, 5, 12, 100, 128])
def test_seg_sum_lengths_against_fp64(cols, accumulate):
    """gi_seg_sum below the four-output threshold: every segment length of SEG_LENGTHS in one CSR, ldv != ldo and both
    above r4(cols); an empty segment gives zero bits (accumulate: the bits of the destination)."""
    c = _sum_case(len(SEG_LENGTHS), cols)
    assert c.cls[0] == 0 and c.cls[1] == 0 and c.cls[-1] == 0 and set(c.cls.tolist()) == set(SEG_LENGTHS)
    _run_seg_sum(c, accumulate, f"seg_sum cols={cols} acc={accumulate}")


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_seg_sum_row_counts_against_fp64(rows):
    """One row; and rows * ceil(cols / 4) one below, at and one above a multiple of the 256 threads of a workgroup."""
    for accumulate in (0, 1):
        _run_seg_sum(_sum_case(rows, 3), accumulate, f"seg_sum rows={rows} cols=3 acc={accumulate}")


def test_seg_sum_no_rows_writes_nothing():
    lib = L.load()
    c = _sum_case(len(SEG_LENGTHS), 5)
    vals = padded(c.vals, 8)
    out = torch.full((4, 8), PAINT, device=DEV)
    for accumulate in (0, 1):
        assert lib.gi_seg_sum(vals.data_ptr(), 8, c.perm_d.data_ptr(), c.off_d.data_ptr(), 0, 5, out.data_ptr(), 8,
                              accumulate, _stream()) == 0
    torch.cuda.synchronize()
    assert painted(out)


# ---- 2. gi_seg_sum, four outputs per thread --------------------------------------------------------------------------
BIG_ROWS, BIG_COLS, BIG_V = 32771, 512, 4096
BIG_SMALL = [0, 1, 2, 3, 4, 5, 6, 7, 9]


def _big_lengths():
    out = [BIG_SMALL[i % 9] for i in range(BIG_ROWS)]
    for i in range(5, BIG_ROWS, 1024):
        out[i] = 33
    for i in range(77, BIG_ROWS, 8192):
        out[i] = 300
    return out


def _chunked_seg_sum(vals, perm, off, rows, base, dtype, chunk=4096):
    parts = []
    for a in range(0, rows, chunk):
        b = min(a + chunk, rows)
        lo, hi = int(off[a]), int(off[b])
        parts.append(SM.seg_sum(vals, perm[lo:hi], off[a:b + 1] - lo, b - a, base=None if base is None else base[a:b],
                                dtype=dtype))
    return torch.cat(parts)


def test_seg_sum_four_outputs_per_thread_against_fp64():
    """rows * ceil(cols / 4) = 32771 * 128 = 4 194 688 threads' worth of outputs: past the 4 << 20 at which gi_seg_sum
    gives every thread four outputs, and no multiple of 1024, so the last workgroup holds threads whose later outputs
    lie beyond the last row.  The same CSR cut to 32767 rows (4 194 176: below the threshold) runs the one-output
    kernel: its rows must be the first launch's rows bit for bit ("bit-identical for every U")."""
    lib = L.load()
    rows, cols, V = BIG_ROWS, BIG_COLS, BIG_V
    c4n = (cols + 3) // 4
    cut = (4 << 20) // c4n - 1
    assert rows * c4n >= (4 << 20) and (rows * c4n) % 1024 != 0 and cut * c4n < (4 << 20) and cut < rows
    g = torch.Generator().manual_seed(77)
    perm, off = SM.csr(_big_lengths(), V, seed=78)
    cls = SM.seg_lengths(off)
    assert set(cls.tolist()) == set(BIG_SMALL) | {33, 300} and set(cls[cut:].tolist()) >= {0, 1, 7, 9}
    sign = column_signs(cols, g)
    vals_h = magnitudes((V, cols), g) * sign
    base_h = magnitudes((rows, cols), g) * sign
    ldv, ldo = cols + 4, cols + 8
    vals = padded(vals_h, ldv)
    perm_d, off_d = perm.to(DEV), off.to(DEV)
    outs = {}
    for name, n, accumulate in (("four", rows, 0), ("one", cut, 0), ("four+acc", rows, 1)):
        out = torch.full((rows + 1, ldo), PAINT, device=DEV)
        if accumulate:
            out[:rows, :cols] = base_h.to(DEV)
        L.check(lib.gi_seg_sum(vals.data_ptr(), ldv, perm_d.data_ptr(), off_d.data_ptr(), n, cols, out.data_ptr(), ldo,
                               accumulate, _stream()), "seg_sum")
        outs[name] = out
    for acc, name in ((0, "four"), (1, "four+acc")):
        base = base_h if acc else None
        r64 = _chunked_seg_sum(vals_h, perm, off, rows, base, F64)
        r32 = _chunked_seg_sum(vals_h, perm, off, rows, base, F32)
        out = outs[name]
        held("seg_sum<4>", f"seg_sum {name} {rows}x{cols}", out[:rows, :cols], r64, r32, cls)
        assert painted(out[:, cols:]) and painted(out[rows])
        if not acc:
            held("seg_sum<1>", f"seg_sum one {cut}x{cols}", outs["one"][:cut, :cols], r64[:cut], r32[:cut], cls[:cut])
    assert painted(outs["one"][cut:]) and painted(outs["one"][:, cols:])
    assert same_bits(outs["one"][:cut], outs["four"][:cut])
    assert zero_bits(outs["four"][(cls == 0).nonzero().flatten().to(DEV), :cols])


# ---- 3. gi_seg_sum_dselu / gi_seg_sum_dselu_f ------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("cols", [1, 5, 100])
def test_seg_sum_dselu_against_fp64(cols, plane):
    """In place on stored outputs of both signs and exact 0.  plane: the factor plane fshift floats behind y is the
    factor (about a quarter exactly 0: the result is a zero) and keeps its bits; without it gi_seg_sum_dselu and
    gi_seg_sum_dselu_f(fshift = 0) are one function.  fshift % 4 != 0 is GI_EINVAL and writes nothing."""
    lib = L.load()
    c = _sum_case(len(SEG_LENGTHS), cols)
    rows, r4 = c.rows, ops.r4(cols)
    assert bool((c.y == 0).any()) and (cols == 1 or (bool((c.y > 0).any()) and bool((c.y < 0).any())))
    ldv, ldy = r4 + 4, r4 + 8
    vals = padded(c.vals, ldv)
    results = []
    for entry in (("f",) if plane else ("plain", "f")):
        buf = with_plane(c.y, c.f, ldy)
        buf_in = buf.clone()
        head = (vals.data_ptr(), ldv, c.perm_d.data_ptr(), c.off_d.data_ptr(), rows, cols, buf.data_ptr(), ldy)
        assert lib.gi_seg_sum_dselu_f(*head, rows * ldy + 2, _stream()) == EINVAL
        torch.cuda.synchronize()
        assert same_bits(buf, buf_in)
        if entry == "plain":
            L.check(lib.gi_seg_sum_dselu(*head, _stream()), "seg_sum_dselu")
        else:
            L.check(lib.gi_seg_sum_dselu_f(*head, rows * ldy if plane else 0, _stream()), "seg_sum_dselu_f")
        y = buf[0]
        held("seg_sum_dselu", f"seg_sum_dselu cols={cols} plane={int(plane)} {entry}", y[:, :cols], c.dact[plane, F64],
             c.dact[plane, F32], c.cls)
        assert same_bits(buf[1], buf_in[1]) and painted(y[:, r4:])
        if plane:
            dropped = (c.f == 0).to(DEV)
            assert bool(dropped.any()) and bool((y[:, :cols][dropped] == 0).all())
        results.append(y.clone())
    assert len(results) == 1 or same_bits(results[0], results[1])


# ---- 4. gi_class_sum_dselu -------------------------------------------------------------------------------------------
# either side of one, two and three turns of the 16 row groups, where the two-loads-in-flight loop starts and ends
CLASS_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 500, 0, 49, 48, 47, 33, 32, 31, 17, 16, 15, 1, 500]
CLASS_V = 600


@pytest.mark.parametrize("problems", [1, 2])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 100])
def test_class_sum_dselu_against_fp64(cols, problems):
    """Two problems in one launch, and one (vals1 = y1 = NULL); pitches above cols; two runs give the same bits;
    columns beyond cols and the row after the last keep their paint."""
    lib = L.load()
    g = torch.Generator().manual_seed(500 + cols)
    rows = len(CLASS_LENGTHS)
    idx, off = SM.csr(CLASS_LENGTHS, CLASS_V, seed=cols)
    cls = SM.seg_lengths(off)
    ldv, ldy = cols + 3, cols + 5
    sign = column_signs(cols, g)
    vals = [magnitudes((CLASS_V, cols), g) * sign for _ in range(2)]
    ys = [stored_outputs((rows, cols), g) for _ in range(2)]
    vals_d = [padded(v, ldv) for v in vals]
    idx_d, off_d = idx.to(DEV), off.to(DEV)
    runs = []
    for _ in range(2):
        y_d = [padded(y, ldy, rows=rows + 1) for y in ys]
        second = problems == 2
        L.check(lib.gi_class_sum_dselu(vals_d[0].data_ptr(), vals_d[1].data_ptr() if second else None, ldv,
                                       idx_d.data_ptr(), off_d.data_ptr(), rows, cols, y_d[0].data_ptr(),
                                       y_d[1].data_ptr() if second else None, ldy, _stream()), "class_sum_dselu")
        runs.append(y_d)
    for k in range(2):
        y = runs[0][k]
        if k < problems:
            held("class_sum_dselu", f"class_sum_dselu cols={cols} problem {k} of {problems}", y[:rows, :cols],
                 SM.class_sum_dact(vals[k], idx, off, ys[k]), SM.class_sum_dact(vals[k], idx, off, ys[k], dtype=F32), cls)
            assert painted(y[:, cols:]) and painted(y[rows])
        else:
            assert same_bits(y, padded(ys[k], ldy, rows=rows + 1))               # not part of the launch
        assert same_bits(runs[0][k], runs[1][k])


# ---- 5. gi_seg_softmax_fwd / gi_seg_softmax_bwd ----------------------------------------------------------------------
SOFTMAX_LENGTHS = [0, 1, 2, 3, 7, 40, 0, 0, 2, 40, 7, 3, 1, 0]
SOFTMAX_V = 48
SOFTMAX_REPEAT = 4                      # this segment (7 slots) lists one message row twice


@functools.lru_cache(maxsize=None)
def _softmax_case(cols, energies):
    g = torch.Generator().manual_seed(600 + cols + len(energies))
    c = types.SimpleNamespace(cols=cols, rows=len(SOFTMAX_LENGTHS))
    c.perm, c.off = SM.csr(SOFTMAX_LENGTHS, SOFTMAX_V, seed=cols, repeat_in=SOFTMAX_REPEAT)
    lo = int(c.off[SOFTMAX_REPEAT])
    assert int(c.perm[lo]) == int(c.perm[lo + 1])
    c.cls = SM.seg_lengths(c.off)
    c.slot_cls = c.cls[SM.slot_segments(c.off)]
    if energies == "randn3":
        c.en = 3 * torch.randn(SOFTMAX_V, cols, generator=g)
    elif energies == "pm100":                               # expf overflows here without the max subtraction
        c.en = (2 * torch.rand(SOFTMAX_V, cols, generator=g) - 1) * 100
        c.en[int(c.perm[lo + 2])] = 100.0                   # (at least one segment surely holds a row above 89)
    else:                                                   # all energies of a segment equal
        c.en = (3 * torch.randn(1, cols, generator=g)).expand(SOFTMAX_V, cols).contiguous()
    c.emb = torch.randn(SOFTMAX_V, cols, generator=g)
    c.dagg = torch.randn(c.rows, cols, generator=g)
    c.fwd = {dt: SM.seg_softmax(c.en, c.emb, c.perm, c.off, dtype=dt)[0] for dt in (F64, F32)}
    c.bwd = {dt: SM.seg_softmax_bwd(c.dagg, c.en, c.emb, c.perm, c.off, dtype=dt) for dt in (F64, F32)}
    assert all(bool(torch.isfinite(t).all()) for dt in (F64, F32) for t in (c.fwd[dt],) + c.bwd[dt])
    c.perm_d, c.off_d = c.perm.to(DEV), c.off.to(DEV)
    return c


SOFTMAX_CASES = [(cols, en) for cols in (1, 7, 20, 100) for en in ("randn3", "pm100", "equal")]


@pytest.mark.parametrize("cols,energies", SOFTMAX_CASES)
def test_seg_softmax_fwd_against_fp64(cols, energies):
    lib = L.load()
    c = _softmax_case(cols, energies)
    rows, r4 = c.rows, ops.r4(cols)
    ld, ldo = r4 + 4, r4 + 8
    en, emb = padded(c.en, ld), padded(c.emb, ld)
    en_in, emb_in = en.clone(), emb.clone()
    out = torch.full((rows + 1, ldo), PAINT, device=DEV)
    L.check(lib.gi_seg_softmax_fwd(en.data_ptr(), emb.data_ptr(), ld, c.perm_d.data_ptr(), c.off_d.data_ptr(), rows, cols,
                                   out.data_ptr(), ldo, _stream()), "seg_softmax_fwd")
    held("seg_softmax_fwd", f"seg_softmax_fwd cols={cols} {energies}", out[:rows, :cols], c.fwd[F64], c.fwd[F32], c.cls)
    assert zero_bits(out[(c.cls == 0).nonzero().flatten().to(DEV), :cols])
    assert painted(out[:, r4:]) and painted(out[rows])
    assert same_bits(en, en_in) and same_bits(emb, emb_in)


@pytest.mark.parametrize("cols,energies", SOFTMAX_CASES)
def test_seg_softmax_bwd_against_fp64(cols, energies):
    """The per-edge rows in slot order, grouped by the length of their segment; the energy gradients of every segment
    sum to zero over its edges (the softmax identity: a wrong <att, emb * dagg> breaks it), held like any other figure:
    within 8 x what the fp32 formulas leave of that sum, floor 1e-6 of the scale of d_en_e in the group (module
    docstring).  A second launch over the CSR without its last three segments leaves their edges' rows painted and gives
    the other rows the same bits."""
    lib = L.load()
    c = _softmax_case(cols, energies)
    rows, r4 = c.rows, ops.r4(cols)
    E = int(c.off[-1])
    ld, ldd, lde = r4 + 4, r4 + 12, r4 + 8
    en, emb, dagg = padded(c.en, ld), padded(c.emb, ld), padded(c.dagg, ldd)
    first = None
    for n in (rows, rows - 3):
        d_en = torch.full((E + 2, lde), PAINT, device=DEV)
        d_emb = torch.full((E + 2, lde), PAINT, device=DEV)
        L.check(lib.gi_seg_softmax_bwd(en.data_ptr(), emb.data_ptr(), ld, c.perm_d.data_ptr(), c.off_d.data_ptr(), n, cols,
                                       dagg.data_ptr(), ldd, d_en.data_ptr(), d_emb.data_ptr(), lde, _stream()),
                "seg_softmax_bwd")
        En = int(c.off[n])
        assert painted(d_en[En:]) and painted(d_emb[En:]) and painted(d_en[:, r4:]) and painted(d_emb[:, r4:])
        if first is None:
            first = (d_en, d_emb)
            assert En == E
        else:
            assert 0 < En < E and same_bits(d_en[:En], first[0][:En]) and same_bits(d_emb[:En], first[1][:En])
    d_en, d_emb = first
    tag = f"seg_softmax_bwd cols={cols} {energies}"
    (en64, emb64), (en32, emb32) = c.bwd[F64], c.bwd[F32]
    seg = SM.slot_segments(c.off)
    att = SM.seg_softmax(c.en, c.emb, c.perm, c.off)[1]
    ed = c.emb.double()[c.perm.long()] * c.dagg.double()[seg]
    inner = torch.zeros(rows, cols, dtype=F64).index_add_(0, seg, att * ed)
    operands = torch.maximum(att * ed.abs(), att * inner[seg].abs()).amax(dim=1)       # d_en_e = att * ed - att * inner
    held("seg_softmax_bwd", f"{tag} d_en_e", d_en[:E, :cols], en64, en32, c.slot_cls, operands=operands)
    held("seg_softmax_bwd", f"{tag} d_emb_e", d_emb[:E, :cols], emb64, emb32, c.slot_cls)
    sums = [torch.zeros(rows, cols, dtype=F64).index_add_(0, seg, t.double())
            for t in (d_en[:E, :cols].cpu(), en32)]
    for k in sorted(set(c.cls.tolist()) - {0}):
        scale = max(float(en64[c.slot_cls == k].abs().max()), float(operands[c.slot_cls == k].max()))
        got = float(sums[0][c.cls == k].abs().max())
        yard = float(sums[1][c.cls == k].abs().max())
        bound = max(8.0 * yard, 1e-6 * scale)
        print(f"{tag} sum of d_en_e over a segment of {k}: kernel {got:.3e} fp32 formulas {yard:.3e} bound {bound:.3e}")
        assert got <= bound, (tag, k)
    assert same_bits(en, padded(c.en, ld)) and same_bits(emb, padded(c.emb, ld)) and same_bits(dagg, padded(c.dagg, ldd))


# ---- 6. gi_selu_bwd_rows_f / gi_selu_bwd_cols3_f ---------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("cols", [1, 5, 128])
def test_selu_bwd_rows_f_against_fp64(cols, gather, inplace, plane):
    """With a gather index that repeats rows and without one, separate and in place on Y, selu' of the stored output
    (gi_selu_bwd_rows and the _f entry with fshift = 0: the same bits) and the factor plane, which keeps its bits."""
    lib = L.load()
    g = torch.Generator().manual_seed(700 + cols)
    rows, src = 37, 11
    idx = torch.randint(0, src, (rows,), generator=g).int() if gather else None
    assert idx is None or idx.unique().numel() < rows
    dY = torch.randn(src if gather else rows, cols, generator=g)
    Y, f = stored_outputs((rows, cols), g), factors((rows, cols), g)
    lddy, ldy = cols + 3, ops.r4(cols) + 4
    ldo = ldy if inplace else cols + 5
    dY_d = padded(dY, lddy)
    idx_d = idx.to(DEV) if gather else None
    r64 = SM.dact_rows(dY, idx, Y, f if plane else None)
    r32 = SM.dact_rows(dY, idx, Y, f if plane else None, dtype=F32)
    results = []
    for entry in (("f",) if plane else ("plain", "f")):
        buf = with_plane(Y, f, ldy)
        buf_in = buf.clone()
        out = buf[0] if inplace else torch.full((rows, ldo), PAINT, device=DEV)
        head = (dY_d.data_ptr(), lddy, idx_d.data_ptr() if gather else None, buf.data_ptr(), ldy, out.data_ptr(), ldo,
                rows, cols)
        if entry == "plain":
            L.check(lib.gi_selu_bwd_rows(*head, _stream()), "selu_bwd_rows")
        else:
            L.check(lib.gi_selu_bwd_rows_f(*head, rows * ldy if plane else 0, _stream()), "selu_bwd_rows_f")
        held("selu_bwd_rows", f"selu_bwd_rows cols={cols} gather={int(gather)} inplace={int(inplace)} plane={int(plane)} "
             f"{entry}", out[:, :cols], r64, r32)
        assert painted(out[:, cols:]) and same_bits(buf[1], buf_in[1]) and same_bits(dY_d, padded(dY, lddy))
        if not inplace:
            assert same_bits(buf[0], buf_in[0])
        if plane:
            assert bool((out[:, :cols][(f == 0).to(DEV)] == 0).all())
        results.append(out[:, :cols].clone())
    assert len(results) == 1 or same_bits(results[0], results[1])


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("widths", [(585, 39, 1), (585, 0, 40), (0, 39, 1), (5, 3, 0)])
def test_selu_bwd_cols3_f_against_fp64(widths, plane):
    """The three column ranges in one launch, with the factor plane and without; a range of width 0 (its pointer NULL)
    writes nothing."""
    lib = L.load()
    g = torch.Generator().manual_seed(800 + widths[0])
    B, W = 7, sum(widths)
    dY, Y, f = torch.randn(B, W, generator=g), stored_outputs((B, W), g), factors((B, W), g)
    lddy, ldy = W + 3, ops.r4(W) + 4
    dY_d, buf = padded(dY, lddy), with_plane(Y, f, ldy)
    buf_in = buf.clone()
    lds = [n + 3 for n in widths]
    outs = [torch.full((B, ld), PAINT, device=DEV) for ld in lds]
    oargs = []
    for n, o, ld in zip(widths, outs, lds):
        oargs += [n, o.data_ptr() if n else None, ld]
    L.check(lib.gi_selu_bwd_cols3_f(dY_d.data_ptr(), lddy, buf.data_ptr(), ldy, B * ldy if plane else 0, B, *oargs,
                                    _stream()), "selu_bwd_cols3_f")
    r64 = SM.dact_rows(dY, None, Y, f if plane else None)
    r32 = SM.dact_rows(dY, None, Y, f if plane else None, dtype=F32)
    start = 0
    for k, (n, o) in enumerate(zip(widths, outs)):
        if n:
            held("selu_bwd_cols3", f"selu_bwd_cols3 {widths} plane={int(plane)} range {k}", o[:, :n],
                 r64[:, start:start + n], r32[:, start:start + n])
        assert painted(o[:, n:])
        start += n
    assert same_bits(buf, buf_in) and same_bits(dY_d, padded(dY, lddy))


# ---- 7. gi_slab_epilogue ---------------------------------------------------------------------------------------------
EPI_FLAGS = [0, SM.EPI_BIAS, SM.EPI_BIAS | SM.EPI_SELU, SM.EPI_DSELU, SM.EPI_MULACT, SM.EPI_DSELU | SM.EPI_ACCUM,
             SM.EPI_MULACT | SM.EPI_ACCUM]


@pytest.mark.parametrize("rows,cols", [(37, 45), (5, 1)])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 8])
def test_slab_epilogue_against_fp64(nsplit, rows, cols):
    """Every flag set the library uses, one slab, an even and an odd count (the even / odd accumulator pair and its
    tail); ld, ldact, ldo and the slab stride all differ and exceed the payload."""
    lib = L.load()
    g = torch.Generator().manual_seed(900 + 10 * nsplit + cols)
    ld, ldact, ldo = cols + 2, cols + 3, cols + 5
    stride = rows * ld + 7
    sign = (torch.randint(0, 2, (1, rows, cols), generator=g) * 2 - 1).float()
    slabs = magnitudes((nsplit, rows, cols), g) * sign
    bias, base = torch.randn(cols, generator=g), torch.randn(rows, cols, generator=g)
    flat = torch.full((nsplit * stride,), PAINT)
    for s in range(nsplit):
        flat[s * stride: s * stride + rows * ld].view(rows, ld)[:, :cols] = slabs[s]
    flat = flat.to(DEV)
    flat_in = flat.clone()
    bias_d = bias.to(DEV)
    for flags in EPI_FLAGS:
        act = factors((rows, cols), g) if flags & SM.EPI_MULACT else stored_outputs((rows, cols), g)
        act_d = padded(act, ldact)
        out = torch.full((rows + 1, ldo), PAINT, device=DEV)
        if flags & SM.EPI_ACCUM:
            out[:rows, :cols] = base.to(DEV)
        uses_act = flags & (SM.EPI_DSELU | SM.EPI_MULACT)
        L.check(lib.gi_slab_epilogue(flat.data_ptr(), nsplit, stride, rows, cols, ld, flags,
                                     bias_d.data_ptr() if flags & SM.EPI_BIAS else None,
                                     act_d.data_ptr() if uses_act else None, ldact, out.data_ptr(), ldo, _stream()),
                "slab_epilogue")
        held("slab_epilogue", f"slab_epilogue {rows}x{cols} nsplit={nsplit} flags={flags}", out[:rows, :cols],
             SM.slab_epilogue(slabs, flags, bias, act, base), SM.slab_epilogue(slabs, flags, bias, act, base, dtype=F32))
        assert painted(out[:, cols:]) and painted(out[rows])
        assert same_bits(flat, flat_in) and same_bits(act_d, padded(act, ldact)) and same_bits(bias_d, bias)


# ---- 8. a CSR without edges ------------------------------------------------------------------------------------------
def test_edgeless_csr():
    """off all zero with a one-element dummy perm: gi_seg_sum gives zero bits (accumulate: leaves the destination's
    bits), the dselu entries y * 0, the softmax forward zero bits, its backward writes nothing.  With perm NULL and no
    edges gi_seg_sum does the same (no slot is ever read: ops.seg_sum passes NULL for an empty index tensor); the other
    entries answer GI_EINVAL and write nothing — the model never gets there: its forward hands them a dummy pointer
    when E == 0, its backward skips the edge branch."""
    lib = L.load()
    g = torch.Generator().manual_seed(1000)
    rows, cols, r4 = 5, 5, 8
    ld = r4 + 4
    off = torch.zeros(rows + 1, dtype=torch.int32, device=DEV)
    dummy = torch.zeros(1, dtype=torch.int32, device=DEV)
    vals = padded(torch.randn(3, cols, generator=g), ld)
    base_h = torch.randn(rows, cols, generator=g)
    y_h, f_h = stored_outputs((rows, cols), g), factors((rows, cols), g)
    for perm in (dummy.data_ptr(), None):
        for accumulate in (0, 1):
            out = torch.full((rows + 1, ld), PAINT, device=DEV)
            if accumulate:
                out[:rows, :cols] = base_h.to(DEV)
            assert lib.gi_seg_sum(vals.data_ptr(), ld, perm, off.data_ptr(), rows, cols, out.data_ptr(), ld, accumulate,
                                  _stream()) == 0
            assert same_bits(out[:rows, :cols], base_h) if accumulate else zero_bits(out[:rows, :cols])
            assert painted(out[:, r4:]) and painted(out[rows])
        for plane in (False, True):
            buf = with_plane(y_h, f_h, ld)
            buf_in = buf.clone()
            rc = lib.gi_seg_sum_dselu_f(vals.data_ptr(), ld, perm, off.data_ptr(), rows, cols, buf.data_ptr(), ld,
                                        rows * ld if plane else 0, _stream())
            rc2 = lib.gi_seg_sum_dselu(vals.data_ptr(), ld, perm, off.data_ptr(), rows, cols, buf.data_ptr(), ld, _stream())
            torch.cuda.synchronize()
            if perm is None:
                assert rc == EINVAL and rc2 == EINVAL and same_bits(buf, buf_in)
            else:
                assert rc == 0 and rc2 == 0 and bool((buf[0][:, :cols] == 0).all())
                assert painted(buf[0][:, r4:]) and same_bits(buf[1], buf_in[1])
        for problems in (1, 2):
            ys = [padded(y_h, ld, rows=rows + 1) for _ in range(2)]
            rc = lib.gi_class_sum_dselu(vals.data_ptr(), vals.data_ptr() if problems == 2 else None, ld, perm,
                                        off.data_ptr(), rows, cols, ys[0].data_ptr(),
                                        ys[1].data_ptr() if problems == 2 else None, ld, _stream())
            torch.cuda.synchronize()
            untouched = padded(y_h, ld, rows=rows + 1)
            if perm is None:
                assert rc == EINVAL and same_bits(ys[0], untouched) and same_bits(ys[1], untouched)
            else:
                assert rc == 0
                for k in range(2):
                    if k < problems:
                        assert bool((ys[k][:rows, :cols] == 0).all()) and painted(ys[k][:, cols:]) and painted(ys[k][rows])
                    else:
                        assert same_bits(ys[k], untouched)
        en, emb = padded(torch.randn(3, cols, generator=g), ld), padded(torch.randn(3, cols, generator=g), ld)
        out = torch.full((rows + 1, ld), PAINT, device=DEV)
        rc = lib.gi_seg_softmax_fwd(en.data_ptr(), emb.data_ptr(), ld, perm, off.data_ptr(), rows, cols, out.data_ptr(),
                                    ld, _stream())
        torch.cuda.synchronize()
        if perm is None:
            assert rc == EINVAL and painted(out)
        else:
            assert rc == 0 and zero_bits(out[:rows, :cols]) and painted(out[:, r4:]) and painted(out[rows])
        dagg = padded(torch.randn(rows, cols, generator=g), ld)
        d_en, d_emb = torch.full((1, ld), PAINT, device=DEV), torch.full((1, ld), PAINT, device=DEV)
        rc = lib.gi_seg_softmax_bwd(en.data_ptr(), emb.data_ptr(), ld, perm, off.data_ptr(), rows, cols, dagg.data_ptr(),
                                    ld, d_en.data_ptr(), d_emb.data_ptr(), ld, _stream())
        torch.cuda.synchronize()
        assert rc == (EINVAL if perm is None else 0) and painted(d_en) and painted(d_emb)
