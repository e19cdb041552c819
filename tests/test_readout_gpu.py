"""-m gpu: the graph-level readout kernels, the gradient sums behind them and FusedAdam against an independent reference
(tests/readout_model.py in fp64), called through the C ABI at the shapes where they change path.

Copies, untouched memory and "exactly 0" are compared as bits.  Everything else: err = max|got - ref64| / max|ref64| of
a tensor must stay within 8 x the err of the same formulas run in fp32 on the CPU for the same case (floor 1e-6, the
bar of one rounded multiply in test_selu_bwd_rows_gather).  The 8 covers the kernels' serial node-order sums against
torch's pairwise ones (about sqrt(128 / 7) ~ 4) and a different expf (x 2).  Where the reference is all zero (de at
N = 1, where a contracted multiply-subtract may leave a rounding residue) an absolute floor takes its place.  Every
figure is printed before it is asserted (pytest -s)."""
import ctypes as C
import functools
import types

import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import ops
from graphinvent_amd.gnn import mpnn
from graphinvent_amd.optim import FusedAdam
from tests import readout_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 1e6
PAINT = 7.0
F32, F64 = torch.float32, torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def painted(t):
    return bool((t == PAINT).all())


def zero_bits(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def held(name, got, ref64, ref32, abs_floor=None):
    """The tolerance of this file (module docstring)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    if scale == 0.0:
        worst = float(got.abs().max()) if got.numel() else 0.0
        limit = 0.0 if abs_floor is None else abs_floor
        print(f"{name}: reference all zero, kernel max {worst:.3e}, limit {limit:.3e}")
        assert worst <= limit, name
        return
    e = float((got - ref64).abs().max()) / scale
    yard = float((ref32.double() - ref64).abs().max()) / scale
    bound = max(8.0 * yard, 1e-6)
    print(f"{name}: kernel {e:.3e} yardstick {yard:.3e} bound {bound:.3e}")
    assert e <= bound, name


def padded(t, ld, rows=None):
    """[rows, ld] on the device, painted, with t in its first columns."""
    buf = torch.full((t.shape[0] if rows is None else rows, ld), PAINT, dtype=F32)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.to(DEV)


def with_plane(t, f, ld):
    """[2, S + 1, ld]: the activations, and the factor plane fshift = (S + 1) * ld floats behind them."""
    assert (t.shape[0] * ld) % 4 == 0
    return torch.stack((padded(t, ld), padded(f, ld)))


def factors(shape, g):
    """AlphaDropout factors: random in [0, 2), about a quarter exactly 0 (dropped units)."""
    return 2 * torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) >= 0.25)


# ---- the batch -------------------------------------------------------------------------------------------------------
A_W, C_W = 45, 3                       # tier-1 widths of the glue entry points
CASES = [(1, 4, 3), (5, 100, 3), (13, 100, 3), (112, 65, 3), (113, 100, 3), (128, 33, 3), (128, 64, 3), (13, 100, 100)]


@functools.lru_cache(maxsize=None)
def _case(N, G, spread):
    """The batch of readout_model.batch_layout(N) with its references, computed once and never written.  Energies are
    3 * randn; spread == 100: uniform over +-100, where expf overflows without the max subtraction."""
    cidx, mask, S = RM.batch_layout(N)
    B = cidx.shape[0]
    g = torch.Generator().manual_seed(7000 + 131 * N + G + spread)
    c = types.SimpleNamespace(N=N, G=G, B=B, S=S, cidx=cidx, mask=mask, cidx_d=cidx.to(DEV), mask_d=mask.to(DEV))
    c.en = 3 * torch.randn(S + 1, G, generator=g) if spread == 3 else (2 * torch.rand(S + 1, G, generator=g) - 1) * 100
    c.emb = torch.randn(S + 1, G, generator=g)
    c.dg = [torch.randn(B, G, generator=g) for _ in range(3)]
    c.f_en, c.f_emb = factors((S + 1, G), g), factors((S + 1, G), g)
    c.t1 = [torch.randn(S + 1, W, generator=g) for W in (A_W, C_W)]
    c.f_t1 = [factors((S + 1, W), g) for W in (A_W, C_W)]
    c.dcat = [torch.randn(B, N * W, generator=g) for W in (A_W, C_W)]
    c.ldG = ops.r4(G) + 4
    c.fwd = {dt: RM.gather_forward(c.en, c.emb, cidx, mask, BIG, dtype=dt) for dt in (F64, F32)}
    c.bwd, c.cmp = {}, {}
    for plane in (False, True):
        for ndg in (1, 3):
            c.bwd[ndg, plane] = {dt: RM.gather_backward(c.en, c.emb, cidx, mask, BIG, S, c.dg[:ndg],
                                                        c.f_en if plane else None, c.f_emb if plane else None, dtype=dt)
                                 for dt in (F64, F32)}
        for k in (0, 1):
            c.cmp[k, plane] = {dt: RM.compress(c.t1[k], cidx, S, c.dcat[k], c.f_t1[k] if plane else None, dtype=dt)
                               for dt in (F64, F32)}
    return c


def _pad_graphs(c):
    return [b for b in range(c.B) if bool((c.cidx[b] == c.S).any())]


# ---- gather forward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["gather", "glue"])
@pytest.mark.parametrize("N,G,spread", CASES)
def test_gather_forward_against_fp64(N, G, spread, entry):
    """gi_gather_readout_fwd, and the same case through gi_readout_glue_fwd: out0 / out1 / out2 at three pitches, all
    given, then each alone with the other two NULL."""
    lib = L.load()
    c = _case(N, G, spread)
    B, ld = c.B, c.ldG
    en, emb = padded(c.en, ld), padded(c.emb, ld)
    pitches = (ops.r4(G) + 4, G + 3, G + 9)
    for given in ((0, 1, 2), (0,), (1,), (2,)):
        outs = [torch.full((B, p), PAINT, device=DEV) for p in pitches]
        oargs = []
        for i in range(3):
            oargs += [outs[i].data_ptr() if i in given else None, pitches[i]]
        gather = (en.data_ptr(), emb.data_ptr(), ld, c.cidx_d.data_ptr(), c.mask_d.data_ptr(), B, N, G, BIG, *oargs)
        if entry == "gather":
            L.check(lib.gi_gather_readout_fwd(*gather, _stream()), "gather_fwd")
        else:
            ldt = [ops.r4(A_W) + 4, ops.r4(C_W)]
            ldc = [N * A_W + 5, N * C_W + 1]
            t1 = [padded(c.t1[k], ldt[k]) for k in (0, 1)]
            cat = [torch.full((B, ldc[k]), PAINT, device=DEV) for k in (0, 1)]
            L.check(lib.gi_readout_glue_fwd(*gather, t1[0].data_ptr(), ldt[0], A_W, cat[0].data_ptr(), ldc[0],
                                            t1[1].data_ptr(), ldt[1], C_W, cat[1].data_ptr(), ldc[1], _stream()),
                    "glue_fwd")
            for k, W in ((0, A_W), (1, C_W)):
                assert same_bits(cat[k][:, :N * W], RM.expand(c.t1[k], c.cidx)) and painted(cat[k][:, N * W:])
        for i in range(3):
            if i in given:
                held(f"fwd N={N} G={G} spread={spread} {entry} out{i} of {given}", outs[i][:, :G], c.fwd[F64], c.fwd[F32])
                assert painted(outs[i][:, G:])
            else:
                assert painted(outs[i])
        assert same_bits(en, padded(c.en, ld)) and same_bits(emb, padded(c.emb, ld))


# ---- gather backward -------------------------------------------------------------------------------------------------
def _check_gather_bwd(tag, c, ndg, plane, en, emb, en_in, emb_in, zbuf):
    G, S, B = c.G, c.S, c.B
    r64, r32 = c.bwd[ndg, plane][F64], c.bwd[ndg, plane][F32]
    dg = sum(d.double() for d in c.dg[:ndg])
    floor = 1e-6 * float(c.emb.abs().max()) * float(dg.abs().max())
    held(f"{tag} en", en[:S, :G], r64[0][:S], r32[0][:S], abs_floor=floor)
    held(f"{tag} emb", emb[:S, :G], r64[1][:S], r32[1][:S])
    z = zbuf[:B * 2 * G].view(B, 2 * G)
    pad = _pad_graphs(c)
    if pad:
        held(f"{tag} zpart(en)", z[pad, :G], r64[2][pad, :G], r32[2][pad, :G], abs_floor=floor)
        held(f"{tag} zpart(emb)", z[pad, G:], r64[2][pad, G:], r32[2][pad, G:])
    full = [b for b in range(B) if b not in pad]
    assert 1 in full and zero_bits(z[full])                 # no padded slot: exactly 0
    assert painted(zbuf[B * 2 * G:])
    # the zero row and every padding column: the input's bits
    assert same_bits(en[S], en_in[S]) and same_bits(emb[S], emb_in[S])
    assert same_bits(en[:, G:], en_in[:, G:]) and same_bits(emb[:, G:], emb_in[:, G:])


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("entry", ["gather", "glue"])
@pytest.mark.parametrize("N,G,spread", CASES)
def test_gather_backward_against_fp64(N, G, spread, entry, plane):
    """gi_gather_readout_bwd_f, and the same case through gi_readout_glue_bwd_f (whose compress half is held to the
    reference too), with dg0 only and with all three dg pointers at three pitches.  plane: the AlphaDropout factor
    plane fshift floats behind every activation is the factor, not selu' of the activation, and stays unchanged."""
    lib = L.load()
    c = _case(N, G, spread)
    B, S, ld = c.B, c.S, c.ldG
    pitches = (ops.r4(G) + 4, G + 3, G + 9)
    dgs = [padded(c.dg[i], pitches[i]) for i in range(3)]
    ldt = [ops.r4(A_W) + 4, ops.r4(C_W)]
    ldc = [N * A_W + 5, N * C_W + 1]
    ldz = [A_W + 3, C_W + 1]
    for ndg in (1, 3):
        tag = f"bwd N={N} G={G} spread={spread} {entry} plane={int(plane)} ndg={ndg}"
        dargs = []
        for i in range(3):
            dargs += [dgs[i].data_ptr() if i < ndg else None, pitches[i]]
        zbuf = torch.full((B * 2 * G + 8,), PAINT, device=DEV)
        if entry == "gather":
            if plane:
                en2, emb2 = with_plane(c.en, c.f_en, ld), with_plane(c.emb, c.f_emb, ld)
                en, emb, fshift = en2[0], emb2[0], (S + 1) * ld
                en2_in, emb2_in = en2.clone(), emb2.clone()
            else:
                en, emb, fshift = padded(c.en, ld), padded(c.emb, ld), 0
            en_in, emb_in = en.clone(), emb.clone()
            L.check(lib.gi_gather_readout_bwd_f(en.data_ptr(), emb.data_ptr(), ld, c.cidx_d.data_ptr(),
                                                c.mask_d.data_ptr(), B, N, G, S, BIG, *dargs, zbuf.data_ptr(), fshift,
                                                _stream()), "gather_bwd")
            if plane:
                assert same_bits(en2[1], en2_in[1]) and same_bits(emb2[1], emb2_in[1])
            _check_gather_bwd(tag, c, ndg, plane, en, emb, en_in, emb_in, zbuf)
            continue
        # one fshift serves all four buffers of the glue launch: they share one region, the factors one region behind
        lds = [ld, ld, ldt[0], ldt[1]]
        offs = [0]
        for x in lds:
            offs.append(offs[-1] + (S + 1) * x)
        region = ops.r4(offs[-1])
        ws = torch.full((2 * region,), PAINT, device=DEV)
        views = []
        for j, (t, f) in enumerate(zip([c.en, c.emb] + c.t1, [c.f_en, c.f_emb] + c.f_t1)):
            for half, src in ((0, t), (1, f)):
                v = ws[half * region + offs[j]: half * region + offs[j + 1]].view(S + 1, lds[j])
                v[:, :src.shape[1]] = src.to(DEV)
                if half == 0:
                    views.append(v)
        ws_in = ws.clone()
        en, emb, t1a, t1b = views
        dcat = [padded(c.dcat[k], ldc[k]) for k in (0, 1)]
        zp = [torch.full((B, ldz[k]), PAINT, device=DEV) for k in (0, 1)]
        L.check(lib.gi_readout_glue_bwd_f(
            en.data_ptr(), emb.data_ptr(), ld, c.cidx_d.data_ptr(), c.mask_d.data_ptr(), B, N, G, S, BIG, *dargs,
            zbuf.data_ptr(), t1a.data_ptr(), ldt[0], A_W, dcat[0].data_ptr(), ldc[0], zp[0].data_ptr(), ldz[0],
            t1b.data_ptr(), ldt[1], C_W, dcat[1].data_ptr(), ldc[1], zp[1].data_ptr(), ldz[1],
            region if plane else 0, _stream()), "glue_bwd")
        assert same_bits(ws[region:], ws_in[region:])                           # the factor region, gaps included
        in_views = [ws_in[offs[j]:offs[j + 1]].view(S + 1, lds[j]) for j in range(4)]
        _check_gather_bwd(tag, c, ndg, plane, en, emb, in_views[0], in_views[1], zbuf)
        for k, W in ((0, A_W), (1, C_W)):
            _check_compress(f"{tag} t1{'ab'[k]}", c, k, plane, views[2 + k], in_views[2 + k], zp[k], W)


# ---- expand / compress -----------------------------------------------------------------------------------------------
def _check_compress(tag, c, k, plane, t1, t1_in, zp, W):
    S = c.S
    r64, r32 = c.cmp[k, plane][F64], c.cmp[k, plane][F32]
    held(f"{tag} rows", t1[:S, :W], r64[0][:S], r32[0][:S])
    assert same_bits(t1[S], t1_in[S]) and same_bits(t1[:, W:], t1_in[:, W:])
    pad = _pad_graphs(c)
    if pad:
        held(f"{tag} zpart", zp[pad, :W], r64[1][pad], r32[1][pad])
    full = [b for b in range(c.B) if b not in pad]
    assert zero_bits(zp[full, :W]) and painted(zp[:, W:])


@functools.lru_cache(maxsize=None)
def _slot_case(N, Wa, Wb):
    cidx, mask, S = RM.batch_layout(N)
    g = torch.Generator().manual_seed(300 + 17 * N + Wa)
    c = types.SimpleNamespace(N=N, B=cidx.shape[0], S=S, cidx=cidx, cidx_d=cidx.to(DEV), W=(Wa, Wb))
    c.t1 = [torch.randn(S + 1, W, generator=g) for W in c.W]
    c.t1[0][1, 0] = 0.0                                      # a stored output of exactly 0: selu' = scale * alpha
    c.f_t1 = [factors((S + 1, W), g) for W in c.W]
    c.dcat = [torch.randn(c.B, N * W, generator=g) for W in c.W]
    c.cmp = {(k, plane): {dt: RM.compress(c.t1[k], cidx, S, c.dcat[k], c.f_t1[k] if plane else None, dtype=dt)
                          for dt in (F64, F32)} for k in (0, 1) for plane in (False, True)}
    return c


SLOT_CASES = [(N, Wa, Wb) for N in (1, 13, 113, 128) for Wa, Wb in ((45, 3), (1, 5))]


@pytest.mark.parametrize("N,Wa,Wb", SLOT_CASES)
def test_expand_slots_is_a_copy(N, Wa, Wb):
    """gi_expand_slots on either width and gi_expand_slots2 on both: bit-exact, painted beyond N * W."""
    lib = L.load()
    c = _slot_case(N, Wa, Wb)
    B = c.B
    ldt = [ops.r4(W) + 4 for W in c.W]
    ldc = [N * Wa + 5, N * Wb + 2]
    t1 = [padded(c.t1[k], ldt[k]) for k in (0, 1)]
    want = [RM.expand(c.t1[k], c.cidx) for k in (0, 1)]
    for pair in (False, True):
        cat = [torch.full((B, ldc[k]), PAINT, device=DEV) for k in (0, 1)]
        if pair:
            L.check(lib.gi_expand_slots2(t1[0].data_ptr(), ldt[0], Wa, cat[0].data_ptr(), ldc[0], t1[1].data_ptr(),
                                         ldt[1], Wb, cat[1].data_ptr(), ldc[1], c.cidx_d.data_ptr(), B, N, _stream()),
                    "expand2")
        else:
            for k in (0, 1):
                L.check(lib.gi_expand_slots(t1[k].data_ptr(), ldt[k], c.cidx_d.data_ptr(), B, N, c.W[k],
                                            cat[k].data_ptr(), ldc[k], _stream()), "expand")
        for k in (0, 1):
            assert same_bits(cat[k][:, :N * c.W[k]], want[k]) and painted(cat[k][:, N * c.W[k]:])


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("N,Wa,Wb", SLOT_CASES)
def test_compress_slots_against_fp64(N, Wa, Wb, plane):
    """gi_compress_slots (no plane) / gi_compress_slots_f on either width and gi_compress_slots2_f on both; at N = 113
    N * Wa crosses 4096 and the four-part grid runs.  One fshift serves both buffers of the pair launch."""
    lib = L.load()
    c = _slot_case(N, Wa, Wb)
    B, S = c.B, c.S
    ldt = [ops.r4(W) + 4 for W in c.W]
    ldc = [N * Wa + 5, N * Wb + 2]
    ldz = [Wa + 3, Wb + 1]
    dcat = [padded(c.dcat[k], ldc[k]) for k in (0, 1)]
    for pair in (False, True):
        tag = f"compress N={N} W={c.W} plane={int(plane)} {'pair' if pair else 'single'}"
        zp = [torch.full((B, ldz[k]), PAINT, device=DEV) for k in (0, 1)]
        if pair:
            offs = [0, (S + 1) * ldt[0], (S + 1) * (ldt[0] + ldt[1])]
            region = offs[2]
            assert region % 4 == 0
            ws = torch.full((2 * region,), PAINT, device=DEV)
            t1 = []
            for k in (0, 1):
                for half, src in ((0, c.t1[k]), (1, c.f_t1[k])):
                    v = ws[half * region + offs[k]: half * region + offs[k + 1]].view(S + 1, ldt[k])
                    v[:, :c.W[k]] = src.to(DEV)
                    if half == 0:
                        t1.append(v)
            ws_in = ws.clone()
            L.check(lib.gi_compress_slots2_f(t1[0].data_ptr(), ldt[0], Wa, dcat[0].data_ptr(), ldc[0], zp[0].data_ptr(),
                                             ldz[0], t1[1].data_ptr(), ldt[1], Wb, dcat[1].data_ptr(), ldc[1],
                                             zp[1].data_ptr(), ldz[1], c.cidx_d.data_ptr(), B, N, S,
                                             region if plane else 0, _stream()), "compress2")
            assert same_bits(ws[region:], ws_in[region:])
            for k in (0, 1):
                _check_compress(f"{tag} {'ab'[k]}", c, k, plane, t1[k], ws_in[offs[k]:offs[k + 1]].view(S + 1, ldt[k]),
                                zp[k], c.W[k])
            continue
        for k in (0, 1):
            buf = with_plane(c.t1[k], c.f_t1[k], ldt[k])
            buf_in = buf.clone()
            head = (buf.data_ptr(), ldt[k], c.cidx_d.data_ptr(), B, N, c.W[k], S, dcat[k].data_ptr(), ldc[k],
                    zp[k].data_ptr(), ldz[k])
            if plane:
                L.check(lib.gi_compress_slots_f(*head, (S + 1) * ldt[k], _stream()), "compress_f")
            else:
                L.check(lib.gi_compress_slots(*head, _stream()), "compress")
            assert same_bits(buf[1], buf_in[1])
            _check_compress(f"{tag} {'ab'[k]}", c, k, plane, buf[0], buf_in[0], zp[k], c.W[k])


# ---- gradient sums ---------------------------------------------------------------------------------------------------
def _coherent(shape, g, sign_dims):
    """Terms in [0.5, 1.5) with one random sign per output element (constant along the summed axis): no sum cancels, so
    err relative to max|ref| also bounds every single output, tensors of one element included."""
    sign = (torch.randint(0, 2, sign_dims, generator=g) * 2 - 1).float()
    return (torch.rand(shape, generator=g) + 0.5) * sign


def _stored_outputs(shape, g):
    """SELU outputs of both signs (> -scale * alpha) with exact zeros among them."""
    y = torch.selu(2 * torch.randn(shape, generator=g))
    y.view(-1)[::3] = 0.0
    return y


COLSUM_ROWS = (0, 1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1000)
COLSUM_COLS = (1, 63, 64, 65, 100)


@pytest.mark.parametrize("ymode", ["null", "separate", "alias"])
def test_colsum_against_fp64(ymode):
    """gi_colsum at the seams of the 16 row groups and of the four-loads-in-flight loop, ldp > cols; y NULL, separate,
    and aliasing out (as the model calls it)."""
    lib = L.load()
    g = torch.Generator().manual_seed(41)
    for rows in COLSUM_ROWS:
        for cols in COLSUM_COLS:
            ldp = cols + 3
            part = _coherent((rows, cols), g, (1, cols))
            y = _stored_outputs((cols,), g)
            part_d = padded(part, ldp, rows=max(rows, 1))
            out = torch.full((cols + 4,), PAINT, device=DEV)
            y_d = None
            if ymode == "separate":
                y_d = y.to(DEV)
            elif ymode == "alias":
                out[:cols] = y.to(DEV)
                y_d = out
            L.check(lib.gi_colsum(part_d.data_ptr(), ldp, rows, cols, y_d.data_ptr() if y_d is not None else None,
                                  out.data_ptr(), _stream()), "colsum")
            yy = None if ymode == "null" else y
            held(f"colsum {ymode} rows={rows} cols={cols}", out[:cols], RM.colsum(part, yy), RM.colsum(part, yy, dtype=F32))
            assert painted(out[cols:])
            if ymode == "separate":
                assert same_bits(y_d, y)


class ColsumDesc(C.Structure):
    """gi_colsum_desc of include/graphinvent_amd.h"""
    _fields_ = [("part", C.c_void_p), ("ldp", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("y", C.c_void_p),
                ("out", C.c_void_p)]


def test_colsum_multi_against_fp64():
    """Four descriptors of different rows and cols in one launch (one with cols = 0, one y NULL, one y aliasing out);
    n = 0 does nothing, n = 9 is GI_EINVAL."""
    lib = L.load()
    g = torch.Generator().manual_seed(42)
    shapes = [(17, 65), (1000, 100), (5, 0), (64, 1)]
    ymodes = ["separate", "alias", "separate", "null"]
    arr = (ColsumDesc * 9)()
    keep, checks = [], []
    for i, ((rows, cols), ymode) in enumerate(zip(shapes, ymodes)):
        ldp = cols + 3
        part = _coherent((rows, cols), g, (1, cols))
        y = _stored_outputs((cols,), g)
        part_d = padded(part, ldp)
        out = torch.full((cols + 4,), PAINT, device=DEV)
        y_d = y.to(DEV) if ymode == "separate" else None
        if ymode == "alias":
            out[:cols] = y.to(DEV)
            y_d = out
        keep += [part_d, out, y_d]
        arr[i].part, arr[i].ldp, arr[i].rows, arr[i].cols = part_d.data_ptr(), ldp, rows, cols
        arr[i].y = y_d.data_ptr() if y_d is not None and cols else None
        arr[i].out = out.data_ptr()
        checks.append((rows, cols, out, part, None if ymode == "null" else y))
    for i in range(4, 9):
        arr[i] = arr[0]
    ptr = C.cast(arr, C.c_void_p)
    assert lib.gi_colsum_multi(ptr, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert painted(checks[0][2]) and painted(checks[3][2])                     # nothing touched yet
    assert lib.gi_colsum_multi(ptr, 9, _stream()) == -1                        # GI_EINVAL
    torch.cuda.synchronize()
    assert painted(checks[0][2]) and painted(checks[3][2])
    L.check(lib.gi_colsum_multi(ptr, 4, _stream()), "colsum_multi")
    for rows, cols, out, part, y in checks:
        if cols:
            held(f"colsum_multi rows={rows} cols={cols}", out[:cols], RM.colsum(part, y), RM.colsum(part, y, dtype=F32))
        assert painted(out[cols:])


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (12, 100)])
def test_slab_sum_dselu_against_fp64(rows, cols):
    """gi_slab_sum_dselu: 16 lanes share an output — nsplit below, at and above 16; pitches and slab stride above the
    payload; destination values of both signs and exactly 0."""
    lib = L.load()
    g = torch.Generator().manual_seed(43 + rows)
    ld, ldy = cols + 2, cols + 5
    stride = rows * ld + 7
    for nsplit in (1, 2, 15, 16, 17, 40):
        slabs = _coherent((nsplit, rows, cols), g, (1, rows, cols))
        y = _stored_outputs((rows, cols), g)
        assert bool((y == 0).any()) and (rows * cols < 3 or (bool((y > 0).any()) and bool((y < 0).any())))
        flat = torch.full((nsplit * stride,), PAINT)
        for s in range(nsplit):
            flat[s * stride: s * stride + rows * ld].view(rows, ld)[:, :cols] = slabs[s]
        flat = flat.to(DEV)
        flat_in = flat.clone()
        y_d = padded(y, ldy)
        L.check(lib.gi_slab_sum_dselu(flat.data_ptr(), nsplit, stride, rows, cols, ld, y_d.data_ptr(), ldy, _stream()),
                "slab_sum_dselu")
        held(f"slab_sum_dselu {rows}x{cols} nsplit={nsplit}", y_d[:, :cols], RM.slab_sum_dselu(slabs, y),
             RM.slab_sum_dselu(slabs, y, dtype=F32))
        assert painted(y_d[:, cols:]) and same_bits(flat, flat_in)


def test_reduce_slabs_against_fp64():
    """gi_reduce_slabs through ops.reduce_slabs: 43 small descriptors (two launches, past the 40 of one table), one
    to three slabs each, one without a bias gradient; what no descriptor owns keeps its paint."""
    g = torch.Generator().manual_seed(44)
    shapes = [(3, 5), (1, 1), (7, 36)]
    n_desc = 43
    no_bias = 41                                             # in the second launch
    specs, size = [], 0
    for i in range(n_desc):
        N, K = shapes[i % 3]
        specs.append((N, K, 1 + (i // 3) % 3, size, size + N * K + 3))
        size += N * K + 3 + N + 2
    out = torch.full((size,), PAINT, device=DEV)
    owned = torch.zeros(size, dtype=torch.bool)
    items, refs = [], []
    for i, (N, K, n_slabs, o_w, o_b) in enumerate(specs):
        ld = K + 1 + 2
        stride = N * ld + 4
        slabs = _coherent((n_slabs, N, K + 1), g, (1, N, K + 1))
        flat = torch.full((n_slabs * stride,), PAINT)
        for s in range(n_slabs):
            flat[s * stride: s * stride + N * ld].view(N, ld)[:, :K + 1] = slabs[s]
        dW = out[o_w:o_w + N * K].view(N, K)
        db = None if i == no_bias else out[o_b:o_b + N]
        owned[o_w:o_w + N * K] = True
        if db is not None:
            owned[o_b:o_b + N] = True
        items.append((flat.to(DEV), dW, db, stride, n_slabs, N, K, ld))
        refs.append((slabs, dW, db))
    assert {(s[0], s[1], s[2]) for s in specs} >= {(N, K, n) for N, K in shapes for n in (1, 2, 3)}
    ops.reduce_slabs(items)
    for i, (slabs, dW, db) in enumerate(refs):
        w64, b64 = RM.reduce_slabs(slabs)
        w32, b32 = RM.reduce_slabs(slabs, dtype=F32)
        held(f"reduce_slabs desc {i} dW", dW, w64, w32)
        if db is not None:
            held(f"reduce_slabs desc {i} db", db, b64, b32)
    assert painted(out.cpu()[~owned]) and int((~owned).sum()) >= 3 * n_desc + specs[no_bias][0]


def test_scale_by_scalar_against_fp64():
    """gi_scale_by_scalar: tails of 1 to 3 floats, n / 4 a multiple of 256 (the tail thread in a block of its own); the
    scale comes from a device scalar; the float after n is not touched."""
    lib = L.load()
    g = torch.Generator().manual_seed(45)
    scale = torch.tensor([0.37], device=DEV)
    for n in (0, 1, 3, 4, 5, 1023, 1024, 1027):
        x0 = torch.randn(n, generator=g)
        x = torch.full((n + 5,), PAINT, device=DEV)
        x[:n] = x0.to(DEV)
        assert x.data_ptr() % 16 == 0
        L.check(lib.gi_scale_by_scalar(x.data_ptr(), n, scale.data_ptr(), _stream()), "scale_by_scalar")
        if n:
            s64 = scale.cpu().double()
            held(f"scale_by_scalar n={n}", x[:n], x0.double() * s64, x0 * scale.cpu())
        assert painted(x[n:])
    assert float(scale) == float(torch.tensor(0.37))


# ---- FusedAdam -------------------------------------------------------------------------------------------------------
ADAM_SHAPES = [(7, 5), (3,), (1,), (64, 9), (2, 2)]
ADAM_GROUPS = [dict(idx=[0, 1, 2], lr=3e-3, weight_decay=1e-2), dict(idx=[3, 4], lr=1e-3, weight_decay=0.0)]


def _adam_setup(seed):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in ADAM_SHAPES]
    frozen = torch.randn(4, 3, generator=g)
    return g, init, frozen


def _fused(init, frozen):
    ps = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    fz = torch.nn.Parameter(frozen.clone().to(DEV), requires_grad=False)
    opt = FusedAdam([dict(params=[ps[i] for i in grp["idx"]] + ([fz] if k == 0 else []), lr=grp["lr"],
                          weight_decay=grp["weight_decay"]) for k, grp in enumerate(ADAM_GROUPS)])
    return ps, fz, opt


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max()) / float(ref.double().abs().max())


def test_fused_adam_skips_and_groups_against_fp64():
    """Two groups of different lr and weight decay, a frozen parameter, eight steps: parameter 1 has no gradient on steps
    3 and 4 (parameter 0 alone, then parameter 2: two launches), parameter 0 none on step 6 (the run starts inside the
    bucket).  Against adam_reference (fp64, the group's step count) and, for the parameters that never skip, against
    torch.optim.Adam on the device, at the 2e-6 of test_fused_adam_matches_torch_adam."""
    g, init, frozen = _adam_setup(51)
    skip = {3: [1], 4: [1], 6: [0]}
    grads = []
    for step in range(1, 9):
        gs = [torch.randn(*s, generator=g) for s in ADAM_SHAPES]
        grads.append([None if i in skip.get(step, []) else x for i, x in enumerate(gs)])
    history = RM.adam_reference(init, ADAM_GROUPS, grads)
    ps, fz, opt = _fused(init, frozen)
    tps = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    topt = torch.optim.Adam([dict(params=[tps[i] for i in grp["idx"]], lr=grp["lr"], weight_decay=grp["weight_decay"])
                             for grp in ADAM_GROUPS])
    where = {}
    for st in opt._flat:
        for p, o in zip(st["params"], st["offs"]):
            where[id(p)] = (st, o)
    assert id(fz) not in where and len(where) == 5

    def state_of(p):
        st, o = where[id(p)]
        return [p.detach().clone(), st["m"][o:o + p.numel()].clone(), st["v"][o:o + p.numel()].clone()]

    for step, (step_grads, (p_ref, m_ref, v_ref)) in enumerate(zip(grads, history), start=1):
        for p, q, gr in zip(ps, tps, step_grads):
            p.grad = None if gr is None else gr.clone().to(DEV)
            q.grad = None if gr is None else gr.clone().to(DEV)
        before = {i: state_of(ps[i]) for i in skip.get(step, [])}
        opt.step(); topt.step()
        for i, old in before.items():                        # a skipped parameter and both its moments: the same bits
            assert all(same_bits(a, b) for a, b in zip(old, state_of(ps[i])))
        for i, p in enumerate(ps):
            _, m, v = state_of(p)
            errs = (_rel(p, p_ref[i]), _rel(m.view_as(p), m_ref[i]), _rel(v.view_as(p), v_ref[i]))
            print(f"adam step {step} param {i}: p {errs[0]:.2e} m {errs[1]:.2e} v {errs[2]:.2e}")
            assert max(errs) < 2e-6
        for i in (2, 3, 4):
            assert _rel(ps[i], tps[i].detach().cpu()) < 2e-6
        assert same_bits(fz.detach(), frozen)
    assert [st["step"] for st in opt._flat] == [8, 8]


def test_fused_adam_reads_a_gradient_bucket_in_place():
    """Gradients that are the views of mpnn.new_grad_bucket are read where they lie (the optimizer hands the kernel the
    bucket itself, not its packed copy) and give the bits that the same gradients in separate tensors give."""
    g, init, frozen = _adam_setup(52)
    ps_a, _, opt_a = _fused(init, frozen)
    ps_b, _, opt_b = _fused(init, frozen)
    buckets = []
    for grp in ADAM_GROUPS:
        members = [ps_b[i] for i in grp["idx"]]
        gflat, views, _ = mpnn.new_grad_bucket(members, DEV)
        for p, v in zip(members, views):
            p.grad = v
        buckets.append(gflat)
    for _ in range(3):
        for p, q in zip(ps_a, ps_b):
            gr = torch.randn(p.shape, generator=g).to(DEV)
            p.grad = gr.clone()
            q.grad.copy_(gr)
        for st_a, st_b, gflat in zip(opt_a._flat, opt_b._flat, buckets):
            assert opt_b._grad_bucket(st_b).data_ptr() == gflat.data_ptr()
            packed = opt_a._grad_bucket(st_a)
            assert packed.data_ptr() == st_a["g"].data_ptr() and packed.data_ptr() != st_a["params"][0].grad.data_ptr()
        opt_a.step(); opt_b.step()
        assert all(same_bits(p.detach(), q.detach()) for p, q in zip(ps_a, ps_b))
    assert not same_bits(ps_a[0].detach(), init[0])
