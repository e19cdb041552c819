"""-m gpu: the draw of gi_sample_actions and gi_sample_actions_rl against an fp64 inverse CDF, where fp32 rounding can
make it go wrong: at the seams between the 256 chunks, at both ends of the CDF and around zero-probability entries.

Rows (tests/sampler_draw_model.make_rows) at W = 625, 3193, 9769 and 15360 (SAMPLE_MAX_W, 256 full chunks of 60):
Gaussian logits at scales 0.3, 3 and 30, a dominant logit, and masked layouts at -inf or max - 200 (a prefix of whole
chunks, a whole wave of chunks, runs across seams, a zero-probability terminate, a ladder of probabilities down to
about 1e-30).  Every finite logit is >= max - 80 or <= max - 200, so "probability 0" means the same in fp32 and fp64.

Uniforms, one per row of a batch that repeats the row: every float32 within K_SEAM ulps of the fp64 CDF at each seam
(subsampled at the wide widths to keep a launch near 512 MB), u = 0, u = 1 - k * 2^-24 for k = 1..64, u = 1, the
midpoints of the first positive entries' intervals, and random u.

Per draw: (a) the index has positive fp64 probability; (b) it does not decrease as u grows; (c) u lies in the index's
fp64 CDF interval widened by Row.tol, the error bound of the kernel's fp32 cumulative sums (<= 1e-5,
tests/test_sampler_draw_cpu.py); (d) it equals oracle.sampler_oracle.draw_inverse_cdf unless u is within that bound
of a boundary; (e) likelihood, like_agent, like_prior and both log-sum-exps match fp64 to 1e-5 relative; (f) the RL
kernel's action, flags, likelihood and index equal the plain kernel's bit for bit, with the agent and prior rows
contiguous, pitched (ld = W + 3) or at a 4-byte offset (scalar loads)."""
import numpy as np
import pytest
import torch

from graphinvent_amd import sampler
from oracle import sampler_oracle as SO
from tests import sampler_draw_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_SEAM = 64
LAUNCH_BYTES = 512 << 20                       # logits bytes of one launch (the repeated agent row)
N_RANDOM = 256
LIKE_REL = 1e-5
LAYOUTS = ("contiguous", "pitched", "offset")


def _flat_index(action, N, A, Fe):
    kind, node, rem = action[:, 0], action[:, 1], action[:, 2]
    return np.where(kind == 0, node * A + rem, np.where(kind == 1, N * A + node * Fe + rem, N * A + N * Fe))


def _prior_row(W, seed):
    """A prior row whose maximum is its last element: the online softmax rescales at the very end."""
    rng = np.random.default_rng([seed, W, 7])
    p = rng.standard_normal(W) * 2.0
    p[-1] = p.max() + 5.0
    return p.astype(np.float32)


def _uniforms(r: M.Row, W, seed):
    rng = np.random.default_rng([seed, W, 11])
    ends = M.end_uniforms()
    pos = np.nonzero(r.e > 0)[0][:8]
    cdf = r.cdf64 / r.total64
    mids = ((np.where(pos > 0, cdf[np.maximum(pos - 1, 0)], 0.0) + cdf[pos]) / 2).astype(np.float32)
    rand = rng.random(N_RANDOM).astype(np.float32)
    seams = np.nonzero(r.hi[:-1] > r.lo[:-1])[0]
    room = LAUNCH_BYTES // (4 * W) - ends.size - mids.size - rand.size
    n_seams = min(seams.size, room // (2 * K_SEAM + 1))
    seams = np.sort(rng.choice(seams, n_seams, replace=False)) if n_seams < seams.size else seams
    return np.concatenate([M.seam_uniforms(r, K_SEAM, seams), ends, mids, rand]).astype(np.float32)


def _batch(row: np.ndarray, n: int, layout: str) -> torch.Tensor:
    """[n, W] on the device, every row equal to `row`, in the given memory layout."""
    W = row.shape[0]
    r = torch.from_numpy(row).to(DEV)
    if layout == "contiguous":
        return r.expand(n, W).contiguous()
    if layout == "pitched":
        buf = torch.zeros((n, W + 3), device=DEV)
        buf[:, :W] = r
        return buf[:, :W]
    buf = torch.zeros((n, W + 4), device=DEV)       # 4 bytes past a 16-byte aligned base: float4 loads are off
    buf[:, 1:W + 1] = r
    return buf[:, 1:W + 1]


def _check_draws(r: M.Row, u: np.ndarray, idx: np.ndarray, what: str) -> list:
    """(a) - (d) for one row: a message per failed property, with its first few draws."""
    W = r.W
    p64 = r.e64 / r.total64
    cdf = r.cdf64 / r.total64
    tol = r.tol()
    u64 = u.astype(np.float64)
    assert np.all((idx >= 0) & (idx < W)), what
    fails = []

    def report(name, sel, extra=None):
        if sel.size:
            msg = f"{name}: {sel.size} of {u.size} draws, u = {u[sel[:4]].tolist()}, idx = {idx[sel[:4]].tolist()}"
            fails.append(msg + (f", {extra(sel[:4])}" if extra else ""))
    # (a) positive probability (logits at max - 200 have fp64 probability < 1e-86: zero on both sides)
    report("(a) zero-probability index", np.nonzero(p64[idx] <= 1e-60)[0])
    # (b) monotone in u
    o = np.argsort(u64, kind="stable")
    report("(b) index decreases as u grows", o[1:][np.diff(idx[o]) < 0])
    # (c) u in [cdf[idx-1], cdf[idx]) widened by the bound
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    lo_tol = np.where(idx > 0, tol[np.maximum(idx - 1, 0)], 0.0)
    report(f"(c) u outside the index's CDF interval +- bound (<= {tol.max():.1e})",
           np.nonzero((u64 < lo - lo_tol) | (u64 > cdf[idx] + tol[idx]))[0])
    # (d) the fp64 inverse CDF, unless u is within the bound of a boundary
    ref = np.concatenate([SO.draw_inverse_cdf(p64[None], u[s])          # one row, broadcast against the u
                          for s in np.array_split(np.arange(u.size), max(1, u.size // 2048))])
    j = np.searchsorted(cdf, u64, side="right")
    t = tol.max()
    near = (np.abs(cdf[np.clip(j - 1, 0, W - 1)] - u64) <= t) | (np.abs(cdf[np.clip(j, 0, W - 1)] - u64) <= t)
    report("(d) differs from the fp64 inverse CDF away from boundaries", np.nonzero((idx != ref) & ~near)[0],
           lambda sel: f"ref = {ref[sel].tolist()}")
    return [f"{what} {m}" for m in fails]


def _rel(a, b):
    return np.abs(a.astype(np.float64) - b) / np.abs(b)


@pytest.mark.parametrize("W", M.WIDTHS)
def test_draw_against_fp64_inverse_cdf(W):
    N, A, Fe = M.dims(W)
    rows = M.make_rows(W)
    problems = []
    for k, (name, logits) in enumerate(rows.items()):
        r = M.Row(logits)
        u = _uniforms(r, W, k)
        n = u.size
        assert n * W * 4 <= LAUNCH_BYTES + (1 << 20)
        what = f"W={W} {name}"
        edges = torch.zeros((n, N, N, Fe), dtype=torch.int8, device=DEV)
        n_nodes = torch.full((n,), min(2, N), dtype=torch.int8, device=DEV)
        ut = torch.from_numpy(u).to(DEV)
        la = _batch(logits, n, "contiguous")
        action, like, flags = sampler.sample_actions_raw(la, n_nodes, edges, A, uniform=ut)
        a = action.cpu().numpy()
        idx = _flat_index(a, N, A, Fe)
        problems += _check_draws(r, u, idx, what)
        # (e) likelihood
        p64 = r.e64 / r.total64
        lk = like.cpu().numpy()
        err = _rel(lk, p64[idx])
        if not np.all(err <= LIKE_REL):
            problems.append(f"{what} (e) likelihood off by {float(np.max(err)):.2e} relative "
                            f"(p64 = {float(p64[idx][np.argmax(err)]):.2e})")
        # the RL kernel on the same agent rows, in one of three layouts, with a prior whose maximum comes last
        layout = LAYOUTS[k % len(LAYOUTS)]
        prior = _prior_row(W, k)
        la2, lp = _batch(logits, n, layout), _batch(prior, n, LAYOUTS[(k + 1) % len(LAYOUTS)])
        a2, la_like, lp_like, f2, idx2, lse = sampler.sample_actions_rl_raw(la2, lp, n_nodes, edges, A, uniform=ut)
        # (f) bit for bit on the agent side
        assert torch.equal(a2, action) and torch.equal(f2, flags) and torch.equal(la_like, like), (what, layout)
        assert np.array_equal(idx2.cpu().numpy(), idx), (what, layout)
        # (e) the prior's probability at the drawn index and both log-sum-exps
        p = prior.astype(np.float64)
        pm = p.max()
        pz = np.exp(p - pm).sum()
        lpl = lp_like.cpu().numpy()
        err = _rel(lpl, np.exp(p[idx] - pm) / pz)
        assert err.max() <= LIKE_REL, (what, "prior", float(err.max()))
        lse_ref = np.array([np.float64(logits.max()) + np.log(r.total64), pm + np.log(pz)])
        lse_err = np.abs(lse.cpu().numpy().astype(np.float64) - lse_ref[None]) / np.maximum(1.0, np.abs(lse_ref))
        assert lse_err.max() <= LIKE_REL, (what, "lse", float(lse_err.max()))
    assert not problems, "\n".join(problems)


def test_draw_covers_tiny_probabilities():
    """The ladder row draws probabilities down to about 1e-30; likelihoods stay within 1e-5 relative there."""
    W = 625
    N, A, Fe = M.dims(W)
    logits = M.make_rows(W)["tiny"]
    r = M.Row(logits)
    cdf = r.cdf64 / r.total64
    p64 = r.e64 / r.total64
    pos = np.nonzero(r.e > 0)[0][:7]
    u = ((np.where(pos > 0, cdf[np.maximum(pos - 1, 0)], 0.0) + cdf[pos]) / 2).astype(np.float32)
    n = u.size
    edges = torch.zeros((n, N, N, Fe), dtype=torch.int8, device=DEV)
    n_nodes = torch.zeros(n, dtype=torch.int8, device=DEV)
    action, like, _ = sampler.sample_actions_raw(_batch(logits, n, "contiguous"), n_nodes, edges, A,
                                                 uniform=torch.from_numpy(u).to(DEV))
    idx = _flat_index(action.cpu().numpy(), N, A, Fe)
    assert np.array_equal(idx, pos)                                  # each midpoint draws its own entry
    assert p64[idx].min() < 1e-29
    assert _rel(like.cpu().numpy(), p64[idx]).max() <= LIKE_REL
