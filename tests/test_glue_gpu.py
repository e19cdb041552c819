"""-m gpu: the GI_GLUE launches (include/graphinvent_amd.h) against the separate launches they replace, compared as bit
patterns: the forward / backward readout glue, the KL loss with its batch mean in the row kernel's launch, the fused GRU
update that aggregates the incoming messages itself, and a tiny GGNN with all four switches off and on."""
import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import loss as loss_mod
from graphinvent_amd import ops, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests.golden.spec import TINY, tiny_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 1e6


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- readout glue ---------------------------------------------------------------------------------------------------
def _glue_case(N):
    """B = 3 graphs of N slots over S compact rows (+ the zero row S): one single-node graph (slot 0), one full graph,
    one whose only node sits in a middle slot — every other slot of graphs 0 and 2 shares the zero row."""
    B, G, A, C = 3, 100, 45, 3
    S = N + 2
    cidx = torch.full((B, N), S, dtype=torch.int32)
    mask = torch.zeros((B, N), dtype=torch.int32)
    cidx[0, 0] = 0; mask[0, 0] = 1
    cidx[1] = torch.arange(1, N + 1, dtype=torch.int32); mask[1] = 1
    cidx[2, N // 2] = N + 1; mask[2, N // 2] = 1
    g = torch.Generator().manual_seed(100 + N)
    ldG, ldA, ldC = ops.r4(G) + 4, ops.r4(A), ops.r4(C)
    t = {"en": torch.randn(S + 1, ldG, generator=g), "emb": torch.randn(S + 1, ldG, generator=g),
         "t1a": torch.randn(S + 1, ldA, generator=g), "t1b": torch.randn(S + 1, ldC, generator=g)}
    ldCA, ldCC = ops.r4(N * A + G) + 4, ops.r4(N * C + G)
    t["dcat_a"] = torch.randn(B, ldCA, generator=g)
    t["dcat_c"] = torch.randn(B, ldCC, generator=g)
    t["dgemb"] = torch.randn(B, ldG, generator=g)
    t = {k: v.to(DEV) for k, v in t.items()}
    return dict(B=B, N=N, G=G, A=A, C=C, S=S, cidx=cidx.to(DEV), mask=mask.to(DEV), ldG=ldG, ldA=ldA, ldC=ldC,
                ldCA=ldCA, ldCC=ldCC, **t)


@pytest.mark.parametrize("N", [5, 113])
def test_readout_glue_forward_is_bitwise_the_two_launches(N):
    """gi_readout_glue_fwd == gi_gather_readout_fwd + gi_expand_slots2: G = 100 is two column chunks of 64 with the
    second partial (four of 32 at N = 113, the GC = 32 path); untouched padding stays untouched."""
    lib = L.load()
    c = _glue_case(N)
    B, G, A, C = c["B"], c["G"], c["A"], c["C"]
    outs = []
    for fused in (False, True):
        cat_a = torch.full((B, c["ldCA"]), 7.0, device=DEV)
        cat_c = torch.full((B, c["ldCC"]), 7.0, device=DEV)
        gemb = torch.full((B, c["ldG"]), 7.0, device=DEV)
        gather = (c["en"].data_ptr(), c["emb"].data_ptr(), c["ldG"], c["cidx"].data_ptr(), c["mask"].data_ptr(), B, N, G,
                  BIG, cat_a.data_ptr() + 4 * N * A, c["ldCA"], cat_c.data_ptr() + 4 * N * C, c["ldCC"],
                  gemb.data_ptr(), c["ldG"])
        expand = (c["t1a"].data_ptr(), c["ldA"], A, cat_a.data_ptr(), c["ldCA"], c["t1b"].data_ptr(), c["ldC"], C,
                  cat_c.data_ptr(), c["ldCC"])
        if fused:
            L.check(lib.gi_readout_glue_fwd(*gather, *expand, _stream()), "glue_fwd")
        else:
            L.check(lib.gi_gather_readout_fwd(*gather, _stream()), "gather_fwd")
            L.check(lib.gi_expand_slots2(*expand, c["cidx"].data_ptr(), B, N, _stream()), "expand2")
        outs.append((cat_a, cat_c, gemb))
    for x, y in zip(*outs):
        assert same_bits(x, y)
    cat_a, cat_c, gemb = outs[1]
    assert bool((cat_a[:, N * A + G:] == 7.0).all()) and bool((gemb[:, G:] == 7.0).all())
    assert bool(torch.isfinite(gemb[:, :G]).all()) and not bool((cat_a[:, :N * A + G] == 7.0).any())


@pytest.mark.parametrize("N", [5, 113])
def test_readout_glue_backward_is_bitwise_the_two_launches(N):
    """gi_readout_glue_bwd_f == gi_gather_readout_bwd_f + gi_compress_slots2_f: the rows overwritten in place and the
    zero-row partial sums of all four stacks (at N = 113 the compress side runs in parts, N * A >= 4096)."""
    lib = L.load()
    c = _glue_case(N)
    B, G, A, C, S = c["B"], c["G"], c["A"], c["C"], c["S"]
    outs = []
    for fused in (False, True):
        en, emb, t1a, t1b = (c[k].clone() for k in ("en", "emb", "t1a", "t1b"))
        zg = torch.full((B, 2 * G), 7.0, device=DEV)
        za = torch.full((B, c["ldA"]), 7.0, device=DEV)
        zc = torch.full((B, c["ldC"]), 7.0, device=DEV)
        gather = (en.data_ptr(), emb.data_ptr(), c["ldG"], c["cidx"].data_ptr(), c["mask"].data_ptr(), B, N, G, S, BIG,
                  c["dgemb"].data_ptr(), c["ldG"], c["dcat_a"].data_ptr() + 4 * N * A, c["ldCA"],
                  c["dcat_c"].data_ptr() + 4 * N * C, c["ldCC"], zg.data_ptr())
        compress = (t1a.data_ptr(), c["ldA"], A, c["dcat_a"].data_ptr(), c["ldCA"], za.data_ptr(), c["ldA"],
                    t1b.data_ptr(), c["ldC"], C, c["dcat_c"].data_ptr(), c["ldCC"], zc.data_ptr(), c["ldC"])
        if fused:
            L.check(lib.gi_readout_glue_bwd_f(*gather, *compress, 0, _stream()), "glue_bwd")
        else:
            L.check(lib.gi_gather_readout_bwd_f(*gather, 0, _stream()), "gather_bwd")
            L.check(lib.gi_compress_slots2_f(*compress, c["cidx"].data_ptr(), B, N, S, 0, _stream()), "compress2")
        outs.append((en, emb, t1a, t1b, zg, za, zc))
    for x, y in zip(*outs):
        assert same_bits(x, y)
    en, emb, t1a, t1b, zg, za, zc = outs[1]
    assert same_bits(en[S], c["en"][S]) and same_bits(t1a[S], c["t1a"][S])          # the zero row is never written
    assert not same_bits(en[:S, :G], c["en"][:S, :G]) and not same_bits(t1a[:S, :A], c["t1a"][:S, :A])
    # the zero-row partial sums: graph 1 has no padded slot, graphs 0 and 2 have N - 1 each
    assert bool((zg[1] == 0).all()) and bool((za[1, :A] == 0).all()) and bool((zc[1, :C] == 0).all())
    assert bool((za[0, :A] != 0).all()) and bool((zc[2, :C] != 0).all()) and bool((zg[2] != 7.0).all())


# ---- KL loss: the batch mean in the row kernel's launch ------------------------------------------------------------------
def _kl_case(B, W, dtype):
    g = torch.Generator().manual_seed(B * 1000 + W)
    out = (torch.randn(B, W, generator=g) * 3).to(DEV)
    tgt = torch.randint(0, 3, (B, W), generator=g)
    tgt[:, 0] = 1
    if B > 1:
        tgt[1] = 0                                   # an all-zero target row: its NaN reaches the mean
    tgt = tgt.to(torch.int8 if dtype == "i8" else torch.float32).to(DEV)
    return out, tgt, (L.DTYPE_I8 if dtype == "i8" else L.DTYPE_F32)


def _kl_call(fn, out, tgt, tdt, stream=None):
    B, W = out.shape
    buf = torch.full((B + 1,), 7.0, device=DEV)
    d_out = torch.full_like(out, 7.0)
    L.check(fn(out.data_ptr(), out.stride(0), tgt.data_ptr(), tdt, tgt.stride(0), B, W, buf.data_ptr(), d_out.data_ptr(),
               d_out.stride(0), buf.data_ptr() + 4 * B, stream if stream is not None else _stream()), "kl")
    return buf, d_out


@pytest.mark.parametrize("dtype", ["i8", "f32"])
@pytest.mark.parametrize("B,W", [(1, 5), (2, 5), (257, 5), (1, 586), (2, 586), (257, 586), (2, 2049)])
def test_kl_loss_mean_is_bitwise_the_two_launches(B, W, dtype):
    """gi_kl_loss_mean == gi_kl_loss (row kernel + mean_rows_kernel): row losses, gradient and mean, NaN of the all-zero
    row included; twice back to back on one stream, then on two streams at once.  At B = 257 thread 0 of the reduction
    sums two rows; W = 2049 takes the 1024-thread row kernel."""
    lib = L.load()
    out, tgt, tdt = _kl_case(B, W, dtype)
    ref_buf, ref_d = _kl_call(lib.gi_kl_loss, out, tgt, tdt)
    if B > 1:
        assert bool(torch.isnan(ref_buf[1])) and bool(torch.isnan(ref_buf[B])) and bool(torch.isfinite(ref_buf[0]))
    else:
        assert bool(torch.isfinite(ref_buf).all())
    got = [_kl_call(lib.gi_kl_loss_mean, out, tgt, tdt) for _ in range(2)]
    torch.cuda.synchronize()
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in side:
        with torch.cuda.stream(s):
            got.append(_kl_call(lib.gi_kl_loss_mean, out, tgt, tdt, s.cuda_stream))
    torch.cuda.synchronize()
    for buf, d in got:
        assert same_bits(buf, ref_buf) and same_bits(d, ref_d)


def test_kl_loss_mean_ring_wraps_and_stays_zeroed():
    """More calls than the ring has words: every word is left zero by the call that used it."""
    lib = L.load()
    out, tgt, tdt = _kl_case(33, 17, "f32")
    ref_buf, _ = _kl_call(lib.gi_kl_loss, out, tgt, tdt)
    got = [_kl_call(lib.gi_kl_loss_mean, out, tgt, tdt)[0] for _ in range(130)]
    torch.cuda.synchronize()
    assert all(same_bits(b, ref_buf) for b in got)


def test_kl_loss_mean_captured_and_replayed():
    lib = L.load()
    out, tgt, tdt = _kl_case(257, 586, "i8")
    ref_buf, ref_d = _kl_call(lib.gi_kl_loss, out, tgt, tdt)
    B, W = out.shape
    buf = torch.full((B + 1,), 7.0, device=DEV)
    d_out = torch.full_like(out, 7.0)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = lib.gi_kl_loss_mean(out.data_ptr(), out.stride(0), tgt.data_ptr(), tdt, tgt.stride(0), B, W,
                                     buf.data_ptr(), d_out.data_ptr(), d_out.stride(0), buf.data_ptr() + 4 * B,
                                     _stream())
    except RuntimeError as e:                                # capture is not available here
        pytest.skip(f"stream capture failed: {e}")
    assert rc == 0
    for _ in range(3):
        buf.fill_(7.0); d_out.fill_(7.0)
        graph.replay()
        eager = _kl_call(lib.gi_kl_loss_mean, out, tgt, tdt)           # an eager call between the replays
        torch.cuda.synchronize()
        assert same_bits(buf, ref_buf) and same_bits(d_out, ref_d)
        assert same_bits(eager[0], ref_buf)


def test_loss_module_uses_the_switch():
    out, tgt, _ = _kl_case(64, 100, "f32")
    tgt[1, 0] = 1
    lib = L.load()
    vals = []
    try:
        for mask in (0, L.GLUE_LOSS_MEAN):
            lib.gi_glue_set(mask)
            o = out.clone().requires_grad_(True)
            l = loss_mod.apd_kl_loss(o, tgt)
            l.backward()
            vals.append((l.detach().clone(), o.grad.clone()))
    finally:
        lib.gi_glue_set(-1)
    assert same_bits(vals[0][0].view(1), vals[1][0].view(1)) and same_bits(vals[0][1], vals[1][1])
    assert bool(torch.isfinite(vals[0][0]))


# ---- fused GRU update with the aggregation inside ----------------------------------------------------------------------
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("H,M", [(128, 128), (64, 32)])
@pytest.mark.parametrize("R", [1, 65, 130])
def test_gru_with_aggregation_is_bitwise_seg_sum_then_gru(R, H, M, bounded):
    """gi_gru_forward_agg == gi_seg_sum + gi_gru_forward: agg, the stored gates, gh_n and h'.  In-degrees cycle through
    5, 0, 1, 2, 3 (no incoming edge: zero and no update; first pair only; pair + tail; two pairs + tail); R = 65 / 130 put
    one / two rows into the second row tile; bounded: the row count comes from the device and is one short of the grid's
    (R = 1: equal) — the rows past it are not touched."""
    lib = L.load()
    g = torch.Generator().manual_seed(R * 7 + H + M)
    Fn = 8
    lda, ldv, ldh, ldg = ops.r4(M) + 4, ops.r4(M) + 8, ops.r4(H + Fn), ops.r4(3 * H) + 4
    deg = torch.tensor([5, 0, 1, 2, 3])[torch.arange(R) % 5]
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).int()
    E = int(seg[-1])
    U = E + 3
    vals = torch.randn(U, ldv, generator=g)
    perm = torch.randint(0, U, (E,), generator=g, dtype=torch.int32)
    hx = torch.randn(R, ldh, generator=g)
    Wih = torch.randn(3 * H, M, generator=g) / M ** 0.5; Whh = torch.randn(3 * H, H, generator=g) / H ** 0.5
    bih = torch.randn(3 * H, generator=g) * 0.3; bhh = torch.randn(3 * H, generator=g) * 0.3
    vals, perm, seg, hx, Wih, Whh, bih, bhh = (t.to(DEV) for t in (vals, perm, seg, hx, Wih, Whh, bih, bhh))
    R_eff = max(R - 1, 1) if bounded else R
    rows_dev = torch.tensor([R_eff], dtype=torch.int32, device=DEV) if bounded else None
    outs = []
    for fused in (False, True):
        agg = torch.full((R, lda), 7.0, device=DEV)
        gi = torch.full((R, ldg), 7.0, device=DEV); gh = torch.full((R, ldg), 7.0, device=DEV)
        hx_new = torch.full((R, ldh), 7.0, device=DEV)
        tail = (hx.data_ptr(), ldh, Wih.data_ptr(), Whh.data_ptr(), bih.data_ptr(), bhh.data_ptr(), gi.data_ptr(),
                gh.data_ptr(), ldg, hx_new.data_ptr(), seg.data_ptr())
        if fused:
            L.check(lib.gi_gru_forward_agg(vals.data_ptr(), ldv, perm.data_ptr(), agg.data_ptr(), lda, *tail, R,
                                           rows_dev.data_ptr() if bounded else None, H, M, _stream()), "gru_agg")
        else:
            L.check(lib.gi_seg_sum(vals.data_ptr(), ldv, perm.data_ptr(), seg.data_ptr(), R_eff, M, agg.data_ptr(), lda,
                                   0, _stream()), "seg_sum")
            L.check(lib.gi_gru_forward(agg.data_ptr(), lda, *tail, R_eff, H, M, _stream()), "gru")
        outs.append((agg, gi, gh, hx_new))
    for x, y in zip(*outs):
        assert same_bits(x, y)
    agg, gi, gh, hx_new = outs[1]
    assert bool((agg[:, M:] == 7.0).all()) and bool((agg[R_eff:] == 7.0).all()) and bool((hx_new[R_eff:] == 7.0).all())
    live = (deg > 0).to(DEV)[:R_eff]
    assert bool((agg[:R_eff, :M][~live] == 0).all()) and bool((gi[:R_eff][~live] == 7.0).all())
    assert same_bits(hx_new[:R_eff][~live], hx[:R_eff][~live])
    assert not bool((gi[:R_eff, :3 * H][live] == 7.0).any())
    # limits are reported
    assert lib.gi_gru_forward_agg(vals.data_ptr(), ldv + 1, perm.data_ptr(), agg.data_ptr(), lda, *tail, R, None, H, M,
                                  _stream()) == -1


# ---- model level -----------------------------------------------------------------------------------------------------
def test_tiny_ggnn_is_bitwise_the_same_with_all_switches_off_and_on():
    """Forward logits, loss and every gradient of a tiny GGNN (two message passes beyond pass 0: the GRU update with the
    aggregation inside runs) with GI_GLUE = 0 and 15."""
    lib = L.load()
    cfg = O.make_config(**TINY)
    assert cfg["message_passes"] >= 2 and cfg["hidden_node_features"] % 4 == 0 and cfg["message_size"] % 4 == 0
    P = O.init_params(cfg, seed=11)
    n8, e8, a8 = tiny_inputs()
    keep = np.nonzero(e8.reshape(e8.shape[0], -1).any(1))[0]
    nodes, edges, tgt = (torch.from_numpy(np.ascontiguousarray(a[keep])).float().to(DEV) for a in (n8, e8, a8))
    results = []
    try:
        for mask in (0, 15):
            assert lib.gi_glue_set(mask) == mask
            model = mpnn.GGNN(O.as_constants(dict(cfg, device="cuda")))
            model.load_state_dict(P)
            model = model.to("cuda").train()
            out = model(nodes, edges)
            l = loss_mod.apd_kl_loss(out, tgt)
            l.backward()
            torch.cuda.synchronize()
            results.append([out.detach().clone(), l.detach().clone().view(1)] +
                           [p.grad.clone() for p in model.parameters()])
    finally:
        lib.gi_glue_set(-1)
    assert len(results[0]) == len(results[1]) > 10
    for a, b in zip(*results):
        assert same_bits(a, b)
    assert bool(torch.isfinite(results[1][1]).all()) and all(bool(torch.isfinite(x).all()) for x in results[1])
