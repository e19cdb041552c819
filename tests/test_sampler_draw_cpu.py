"""The sampler's claim rule, restated on the CPU (tests/sampler_draw_model.py), at the four widths the GPU tests use:
  * the fixed rule: every float32 target in windows around every chunk seam and in the whole tail up to the total has
    exactly one owning chunk, draws an index with e > 0, and the index never decreases as the target grows; the total
    itself draws the last index with e > 0;
  * the rule it replaced shows the misses: targets at the seams that no chunk claims (terminate is returned far from
    the end of the CDF) and zero-probability draws;
  * the bound the GPU tests allow: every fp32 boundary lies within Row.tol of the fp64 CDF, Row.tol stays under 1e-5,
    and the seam sweep's K covers the fp32 / fp64 offset twice over."""
import numpy as np
import pytest

from tests import sampler_draw_model as M

K_SEAM = 64                                            # ulps of u swept on either side of a seam (GPU tests)
TAIL = 1 << 14                                         # float32 targets just below the total, all of them


def _window(x: np.ndarray, k: int) -> np.ndarray:
    """All float32 within k ulps of each x (non-negative)."""
    bits = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    w = np.clip((bits[:, None] + np.arange(-k, k + 1)[None]).reshape(-1), 0, None)
    return np.unique(w.astype(np.int32).view(np.float32))


def _targets(r: M.Row) -> np.ndarray:
    """Windows of 64 ulps around both rules' chunk boundaries and walk ends, the whole tail, and 0, clipped to
    [0, total] and sorted."""
    n = r.hi - r.lo
    live = n > 0
    ends = np.concatenate([r.B, r.incl, r.excl_old[live], r.walk[live, np.maximum(n[live] - 1, 0)],
                           r.walk_old[live, np.maximum(n[live] - 1, 0)]])
    tb = r.total.view(np.int32)
    tail = (tb - np.arange(TAIL, dtype=np.int32)).view(np.float32)
    t = np.concatenate([_window(ends, 64), tail, [0.0], [r.total]]).astype(np.float32)
    return np.unique(t[(t >= 0) & (t <= r.total)])


@pytest.mark.parametrize("W", M.WIDTHS)
def test_fixed_rule_claims_every_target_once_monotone_and_positive(W):
    for name, logits in M.make_rows(W).items():
        r = M.Row(logits)
        t = _targets(r)
        assert np.all(r.owners(t) == 1), name
        idx = r.draw(t)
        assert np.all((idx >= 0) & (idx < W)), name
        assert np.all(r.e[idx] > 0), name
        assert np.all(np.diff(idx) >= 0), name                       # t is sorted
        assert idx[-1] == np.nonzero(r.e > 0)[0][-1], name            # the total: the last e > 0
        assert idx[0] == np.nonzero(r.e > 0)[0][0], name              # 0: the first e > 0
        # past the total (u * total cannot get there, the rule must still hold)
        assert r.draw(np.array([np.nextafter(r.total, np.float32(np.inf))]))[0] == idx[-1]


def test_replaced_rule_misses_at_seams_and_in_the_tail():
    seam_misses = zero_draws = 0
    for W in M.WIDTHS:
        for name, logits in M.make_rows(W).items():
            r = M.Row(logits)
            t = _targets(r)
            old = r.draw_old(t)
            cdf_before_last = float(r.cdf64[W - 2] / r.total64)
            far = t / float(r.total) < cdf_before_last - r.tol()[W - 2]
            seam_misses += int(np.sum((old == W - 1) & far))
            zero_draws += int(np.sum(r.e[old] == 0))
    assert seam_misses > 0, "the replaced rule should return terminate at some seam far from the CDF's end"
    assert zero_draws > 0, "the replaced rule should draw a zero-probability terminate"


@pytest.mark.parametrize("W", M.WIDTHS)
def test_fp32_boundaries_lie_within_the_stated_bound(W):
    for name, logits in M.make_rows(W).items():
        r = M.Row(logits)
        tol = r.tol()
        cdf = r.cdf64 / r.total64
        off = np.abs(r.fp32_boundaries() - cdf[None]).max(axis=0)
        assert np.all(off <= tol), name
        assert tol.max() <= 1e-5, (name, tol.max())                   # no looser than the bound it replaces
        ulp = np.spacing(np.maximum(cdf, 1e-30).astype(np.float32)).astype(np.float64)
        assert (off / ulp)[r.e > 0].max() <= K_SEAM / 2, name         # the seam sweep covers the offset


def test_seam_and_end_uniforms_cover_what_they_claim():
    r = M.Row(M.make_rows(625)["scale3"])
    u = M.seam_uniforms(r, K_SEAM)
    assert u.size == (np.count_nonzero(r.hi[:-1] > r.lo[:-1])) * (2 * K_SEAM + 1)
    e = M.end_uniforms()
    assert e[0] == 0 and e[-1] == 1 and e[1] == np.nextafter(np.float32(1), np.float32(0))
    assert np.all(np.diff(e[1:-1]) < 0) and e.dtype == np.float32
