"""-m gpu: the column-split fp16x2 forward / dgrad kernel (csrc/gi_gemm_x2n.hip) against the kernel it replaces
(gi_gemm_bf3_kernel's fp16x2 form, reached with GI_X2N=0): bit for bit at the node-level shapes of the model — outputs,
the untouched margins of C, every slot of the c_amax cell and the dynamic-range guard's count — on bounded launches
(m_dev below M), unbounded ones (the old kernel then walked its tiles in XCD order), N and K of 250 and 500, K not a
multiple of 32, and rows planted below the guard's range."""
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = L.GEMM_BF3 | L.GEMM_BF3B_F32 | L.GEMM_X2


def _make(shapes, m_cap, seed, low_rows=0, dgrad=False):
    """One launch's problems: shapes = [(N, K)], A [m_cap, r4(K)], B [N, ldb] fp32 with NaN beyond K (never read),
    amax cells from gi_absmax as the model's producers would leave them."""
    g = torch.Generator().manual_seed(seed)
    probs = []
    for i, (n, k) in enumerate(shapes):
        lda, ldb, ldc = ops.r4(k), k + 4 * (i % 2), ops.r4(n) + 4
        A = torch.randn(m_cap, lda, generator=g)
        A[:, k:] = float("nan")
        if low_rows:                                  # below 2^-24 of the tensor's maximum: the guard's low rows
            A[torch.randperm(m_cap, generator=g)[:low_rows], :k] *= 1e-9
        B = torch.randn(n, ldb, generator=g) / k ** 0.5
        B[:, k:] = float("nan")
        bias = torch.randn(n, generator=g)
        act = torch.randn(m_cap, ldc, generator=g)
        cells = torch.zeros(2, L.AMAX_WORDS, device=DEV)
        Ad, Bd = A.to(DEV), B.to(DEV)
        ops.absmax([Ad[:, :k], Bd[:, :k]], cells)
        probs.append(dict(A=Ad, B=Bd, bias=bias.to(DEV), act=act.to(DEV), cells=cells, n=n, k=k,
                          lda=lda, ldb=ldb, ldc=ldc))
    return probs


def _run(probs, m_cap, m_dev, dgrad, old):
    """One gi_gemm_batch launch; returns (C of every problem, c_amax cells, guard count)."""
    os.environ["GI_X2N"] = "0" if old else "1"
    b3p_all = os.environ.pop("GI_B3P_ALL", None)        # (another test's switch: would route these to gi_b3p_kernel)
    try:
        n = len(probs)
        arr = (L.GemmParams * n)()
        outs, camax = [], torch.zeros(n, L.AMAX_WORDS, device=DEV)
        guard = torch.zeros(1, dtype=torch.int32, device=DEV)
        for i, q in enumerate(probs):
            Cd = torch.full((m_cap, q["ldc"]), 7.0, device=DEV)
            outs.append(Cd)
            p = arr[i]
            p.A, p.B, p.C = q["A"].data_ptr(), q["B"].data_ptr(), Cd.data_ptr()
            p.M, p.N, p.K, p.lda, p.ldb, p.ldc = m_cap, q["n"], q["k"], q["lda"], q["ldb"], q["ldc"]
            p.nsplit = 1
            if dgrad:
                p.flags = L.EPI_DSELU | F
                p.act, p.ldact = q["act"].data_ptr(), q["ldc"]
            else:
                p.flags = L.EPI_BIAS | L.EPI_SELU | F
                p.bias = q["bias"].data_ptr()
            p.m_dev = m_dev.data_ptr() if m_dev is not None else None
            p.a_amax, p.b_amax = q["cells"][0].data_ptr(), q["cells"][1].data_ptr()
            p.c_amax = camax[i].data_ptr()
            p.x2_guard = guard.data_ptr()
        L.check(L.load().gi_gemm_batch(arr, n, ops._stream()), "gi_gemm_batch")
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs], camax.cpu().numpy(), int(guard.item())
    finally:
        os.environ.pop("GI_X2N", None)
        if b3p_all is not None:
            os.environ["GI_B3P_ALL"] = b3p_all


NODE = [(500, 500), (500, 500), (250, 250), (250, 250)]       # the readout's four sibling MLPs' hidden layers


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("shapes,m_cap,m_real,low", [
    (NODE, 7355, 7000, 0),                 # bounded: m_dev < M
    (NODE, 7355, None, 0),                 # unbounded, >= 512 tiles: the old kernel's XCD order (c_amax slots)
    (NODE, 2600, 2601, 37),                # m_dev above M; planted low rows
    ([(500, 136), (250, 250), (384, 20)], 1000, 999, 5),     # K of 136 / 20: a partial or single 32-deep step
    ([(128, 64), (500, 500)], 300, None, 0),                   # K a multiple of 32, < 512 tiles
])
def test_x2n_kernel_bitwise_equals_the_kernel_it_replaces(shapes, m_cap, m_real, low, dgrad):
    probs = _make(shapes, m_cap, seed=m_cap + len(shapes) + low, low_rows=low, dgrad=dgrad)
    m_dev = torch.tensor([m_real], dtype=torch.int32, device=DEV) if m_real is not None else None
    new = _run(probs, m_cap, m_dev, dgrad, old=False)
    old = _run(probs, m_cap, m_dev, dgrad, old=True)
    rows = m_cap if m_real is None else min(m_cap, m_real)
    for i, q in enumerate(probs):
        assert np.array_equal(new[0][i], old[0][i], equal_nan=True), i
        assert np.array_equal(new[0][i].view(np.uint32), old[0][i].view(np.uint32)), i
        assert np.isfinite(new[0][i][:rows, :q["n"]]).all()
        assert (new[0][i][rows:] == 7.0).all() and (new[0][i][:, q["n"]:] == 7.0).all()
        assert float(new[1][i].max()) == float(np.abs(new[0][i][:rows, :q["n"]]).max())
    assert np.array_equal(new[1].view(np.uint32), old[1].view(np.uint32))       # every slot of every cell
    assert new[2] == old[2]
    if low:
        assert new[2] > 0
