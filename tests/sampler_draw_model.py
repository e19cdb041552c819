"""CPU restatement of the draw in ``csrc/gi_sample.hip`` (``sample_actions_kernel``) in numpy float32: the kernel's
chunking, scan and walk order, for the fixed claim rule (``draw``) and for the rule it replaced (``draw_old``).
numpy's float32 ``exp`` stands in for the device ``expf``; they differ in the last bits, which moves individual seams
but not the shape of the rule.

The kernel, per row of width W: ``e = expf(l - max)``; 256 chunks of ``L = ceil(W / 256)`` contiguous elements;
``csum(t)`` is the sequential sum of chunk t; an inclusive scan of the chunk sums (a Hillis-Steele scan with wave
shuffles inside each 64-lane wave, then the wave totals added in wave order) gives ``woff + x``, whose last value is
``total``; ``target = fl(u * total)``.  The fixed rule's chunk boundaries are ``B(t)``, the running maximum of
``woff + x`` clamped to ``total``: ``woff + x`` itself can step down after a chunk of zeros, because the scan's
intermediate window sums are not monotone.

Besides the fp32 values, ``Row`` carries a running bound on the error of every cumulative value against the fp64
cumulative sum of the fp64 softmax numerators ``exp(l - max)``: each fp32 addition ``z = a + b`` of non-negative
terms adds ``|z| * 2^-24`` to the bounds of its operands, and each ``e`` starts with ``e * (|fl(l - max) - (l - max)|
+ 2^-22)`` (the rounding of the subtraction, and two ulps for ``expf``).  ``Row.tol`` turns these into the bound on
``|u - cdf64|`` at every boundary that the GPU tests allow.
"""
from __future__ import annotations

import numpy as np

THREADS = 256
WAVE = 64
EPS = 2.0 ** -24                      # unit roundoff of float32
EXP_REL = 2.0 ** -22                  # allowance for the device expf: 2 ulps, relative


def chunk_bounds(W: int):
    L = -(-W // THREADS)
    lo = np.minimum(np.arange(THREADS) * L, W)
    return L, lo, np.minimum(lo + L, W)


class Row:
    """One logits row through the kernel's arithmetic (fp32 values, fp64 error bounds)."""

    def __init__(self, logits: np.ndarray):
        l32 = np.asarray(logits, dtype=np.float32)
        W = l32.shape[0]
        self.W = W
        self.L, self.lo, self.hi = chunk_bounds(W)
        L = self.L
        mx = l32.max()
        d32 = l32 - mx                                      # fp32 subtraction, as in the kernel
        d64 = l32.astype(np.float64) - np.float64(mx)
        self.e = np.exp(d32).astype(np.float32)
        self.e64 = np.exp(d64)
        with np.errstate(invalid="ignore"):                 # -inf - -inf at masked entries: no error there
            derr = np.where(np.isfinite(d64), np.abs(d32.astype(np.float64) - d64), 0.0)
        eb = self.e.astype(np.float64) * (derr + EXP_REL)
        # chunk layout [256, L], zero-padded past W (padding never enters a sum: it is masked below)
        pad = np.zeros(THREADS * L, dtype=np.float32)
        pad[:W] = self.e
        padb = np.zeros(THREADS * L)
        padb[:W] = eb
        ec, ebc = pad.reshape(THREADS, L), padb.reshape(THREADS, L)
        n = self.hi - self.lo
        csum = np.zeros(THREADS, dtype=np.float32)
        cb = np.zeros(THREADS)
        for j in range(L):
            on = j < n
            csum = np.where(on, csum + ec[:, j], csum).astype(np.float32)
            cb = np.where(on, cb + ebc[:, j] + np.abs(csum.astype(np.float64)) * EPS, cb)
        self.csum = csum
        # wave scan: x <- x + shfl_up(x, o) for lanes >= o, o = 1, 2, ..., 32 (all lanes at once)
        x, xb = csum.reshape(4, WAVE).copy(), cb.reshape(4, WAVE).copy()
        o = 1
        while o < WAVE:
            y, yb = x.copy(), xb.copy()
            x[:, o:] = (y[:, o:] + y[:, :-o]).astype(np.float32)
            xb[:, o:] = yb[:, o:] + yb[:, :-o] + np.abs(x[:, o:].astype(np.float64)) * EPS
            o <<= 1
        wtot, wtb = x[:, WAVE - 1], xb[:, WAVE - 1]
        woff = np.zeros(4, dtype=np.float32)
        wob = np.zeros(4)
        for w in range(1, 4):
            woff[w] = np.float32(woff[w - 1] + wtot[w - 1])
            wob[w] = wob[w - 1] + wtb[w - 1] + abs(float(woff[w])) * EPS
        incl = (woff[:, None] + x).astype(np.float32).reshape(-1)      # woff + x
        inclb = (wob[:, None] + xb).reshape(-1) + np.abs(incl.astype(np.float64)) * EPS
        self.total = np.float32(np.float32(np.float32(wtot[0] + wtot[1]) + wtot[2]) + wtot[3])
        assert self.total == incl[-1]                       # the same additions in the same order
        self.total_b = inclb[-1]
        self.incl = incl
        # the boundaries: running maximum of woff + x (not monotone itself), clamped to the total; a maximum or a
        # minimum picks one of the values it compares, so its bound is the largest of theirs
        self.B = np.minimum(np.maximum.accumulate(incl), self.total).astype(np.float32)
        self.Bb = np.maximum(np.maximum.accumulate(inclb), self.total_b)
        self.bprev = np.concatenate([[np.float32(0)], self.B[:-1]]).astype(np.float32)
        self.bprevb = np.concatenate([[0.0], self.Bb[:-1]])
        # the old rule's exclusive prefix: (woff + x) - csum
        self.excl_old = (incl - csum).astype(np.float32)
        # running sums of the walks: new from B(t-1), old from excl_old(t)
        self.walk = self._walk(self.bprev, ec, n)
        self.walk_old = self._walk(self.excl_old, ec, n)
        wb = np.empty((THREADS, L))
        c = self.bprevb.copy()
        for j in range(L):
            c = c + ebc[:, j] + np.abs(self.walk[:, j].astype(np.float64)) * EPS
            wb[:, j] = c
        self.walkb = wb
        # last index with e > 0 at or before the end of each chunk (-1: none)
        pos = np.where(self.e > 0, np.arange(W), -1)
        lastpos = np.full(THREADS, -1)
        for t in range(THREADS):
            if n[t] > 0:
                lastpos[t] = pos[self.lo[t]:self.hi[t]].max()
        self.upto = np.maximum.accumulate(lastpos)
        # fp64 reference: the cumulative sum of exp(l - max), and its total
        self.cdf64 = np.cumsum(self.e64)
        self.total64 = self.cdf64[-1]

    def _walk(self, start, ec, n):
        c = start.astype(np.float32).copy()
        out = np.empty(ec.shape, dtype=np.float32)
        for j in range(ec.shape[1]):
            c = np.where(j < n, c + ec[:, j], c).astype(np.float32)
            out[:, j] = c
        return out

    # ---- targets ---------------------------------------------------------------------------------------------------
    def targets(self, u: np.ndarray) -> np.ndarray:
        return (np.asarray(u, dtype=np.float32) * self.total).astype(np.float32)

    def owners(self, target: np.ndarray) -> np.ndarray:
        """How many chunks claim each target under the fixed rule (the kernel needs exactly one)."""
        t = np.asarray(target, dtype=np.float32)[:, None]
        last = np.arange(THREADS) == THREADS - 1
        return ((self.bprev[None] <= t) & ((t < self.B[None]) | last[None])).sum(axis=1)

    def draw(self, target: np.ndarray) -> np.ndarray:
        """The fixed rule: chunk t owns [B(t-1), B(t)) (the last chunk also everything past it); inside, the first
        element whose running sum exceeds the target, else the last element with e > 0 at or before the chunk's end."""
        tg = np.asarray(target, dtype=np.float32)
        t = np.minimum(np.searchsorted(self.B, tg, side="right"), THREADS - 1)
        inside = tg < self.B[t]
        n = (self.hi - self.lo)[t]
        k = (self.walk[t] <= tg[:, None]).sum(axis=1)       # leading elements whose running sum is <= target
        found = inside & (k < n)
        return np.where(found, self.lo[t] + k, self.upto[t])

    def draw_old(self, target: np.ndarray) -> np.ndarray:
        """The replaced rule: every chunk with excl_old <= target walks from excl_old; the smallest index whose running
        sum exceeds the target wins; no find -> W - 1."""
        tg = np.asarray(target, dtype=np.float32)
        n = self.hi - self.lo
        cend = self.walk_old[np.arange(THREADS), np.maximum(n - 1, 0)]
        finds = (n[None] > 0) & (self.excl_old[None] <= tg[:, None]) & (tg[:, None] < cend[None])
        any_ = finds.any(axis=1)
        t = np.argmax(finds, axis=1)
        k = (self.walk_old[t] <= tg[:, None]).sum(axis=1)
        return np.where(any_, self.lo[t] + k, self.W - 1)

    # ---- the bound ---------------------------------------------------------------------------------------------------
    def tol(self) -> np.ndarray:
        """Per index j: a bound on |fp32 boundary / total - cdf64[j] / total64| over every fp32 expression of the
        cumulative sum up to j that the rule compares a target with (the walk value, and B(t) at a chunk's end), plus
        the rounding of u * total.  Dividing by the fp32 total instead of the fp64 one adds the total's bound."""
        W, L = self.W, self.L
        wb = self.walkb.reshape(-1)[:W].copy()
        n = self.hi - self.lo
        ends = self.hi[n > 0] - 1
        wb[ends] = np.maximum(wb[ends], self.Bb[n > 0])
        # a zero-probability element carries the bound of the last positive one before it (same cumulative value)
        wb = np.maximum.accumulate(wb)
        return 1.01 * (wb + self.total_b) / float(self.total) + 2 * EPS

    def fp32_boundaries(self) -> np.ndarray:
        """Every fp32 cumulative value the rule can compare against, per index, over total: the walk value and, at the
        end of a chunk, B(t) too.  Returns [2, W] (the second row repeats the walk value off the chunk ends)."""
        W = self.W
        wv = self.walk.reshape(-1)[:W].astype(np.float64)
        bv = wv.copy()
        n = self.hi - self.lo
        bv[self.hi[n > 0] - 1] = self.B[n > 0]
        return np.stack([wv, bv]) / float(self.total)


# ---- test rows -------------------------------------------------------------------------------------------------------
WIDTHS = (625, 3193, 9769, 15360)     # GDB-13 fixture (N = 13), a mid width, ChEMBL (N = 88), SAMPLE_MAX_W (L = 60)
ZERO_GAP = 200.0                      # masked logits sit at max - 200 (or -inf): exp underflows to 0 in fp32
LIVE_GAP = 80.0                       # every other finite logit is >= max - 80: a normal fp32 exp, > 0 in both


def dims(W: int):
    """(N, A, Fe) with N * A + N * Fe + 1 = W."""
    return {625: (13, 45, 3), 3193: (24, 130, 3), 9769: (88, 108, 3), 15360: (1, 15356, 3)}[W]


def _enforce(l: np.ndarray) -> np.ndarray:
    """Move every finite logit in (max - 200, max - 80) to max - 200, so "probability 0" means the same in fp32 and
    fp64."""
    l = l.astype(np.float32)
    mx = np.float32(l.max())
    mid = np.isfinite(l) & (l > mx - ZERO_GAP) & (l < mx - LIVE_GAP)
    l[mid] = np.float32(mx - ZERO_GAP)
    return l


def make_rows(W: int, seed: int = 0) -> dict:
    """Seeded logits rows of width W: Gaussian at three scales, a dominant logit, and masked layouts (a prefix of
    whole chunks, a whole wave of chunks, runs straddling seams, a zero-probability terminate, and a ladder of
    probabilities down to about 1e-30 behind a masked prefix)."""
    rng = np.random.default_rng([seed, W])
    L, lo, hi = chunk_bounds(W)
    g = lambda s: rng.standard_normal(W) * s                 # noqa: E731
    rows = {"scale0.3": g(0.3), "scale3": g(3.0), "scale30": g(30.0)}
    d = g(1.0)
    d[rng.integers(W)] = 40.0
    rows["dominant"] = d
    p = g(3.0)
    p[:5 * L + 2] = -np.inf                                   # five whole chunks and two more elements
    rows["prefix"] = p
    w = g(3.0)
    w[64 * L:128 * L] = w.max() - ZERO_GAP                    # chunks 64..127: the whole second wave
    rows["wave"] = w
    s = g(3.0)
    mx = s.max()
    for k, t in enumerate(range(2, THREADS - 1, 5)):           # runs of 5 across the seam after chunk t
        if hi[t] + 3 <= W - 1:
            s[hi[t] - 2:hi[t] + 3] = -np.inf if k % 2 else mx - ZERO_GAP
    rows["straddle"] = s
    z = g(3.0)
    z[-3:-1] = z.max() - ZERO_GAP
    z[-1] = -np.inf                                           # terminate (and the two before it) at probability 0
    rows["term0"] = z
    t = g(3.0)
    t[:2 * L] = -np.inf
    ladder = np.array([69.0, 58.0, 46.0, 35.0, 23.0, 12.0, 4.0])
    t[2 * L:2 * L + ladder.size] = t.max() - ladder           # p ~ 1e-30 ... behind two masked chunks
    rows["tiny"] = t
    return {k: _enforce(v) for k, v in rows.items()}


def seam_uniforms(row: Row, K: int, seams=None) -> np.ndarray:
    """Every float32 u within K ulps of cdf64(end of chunk t) / total64, for each seam t (all by default)."""
    n = row.hi - row.lo
    ts = np.nonzero(n[:-1] > 0)[0] if seams is None else np.asarray(seams)
    u0 = (row.cdf64[row.hi[ts] - 1] / row.total64).astype(np.float32)
    return ulp_window(u0, K)


def ulp_window(x0: np.ndarray, K: int) -> np.ndarray:
    """All float32 within K ulps of each x0 (non-negative), flattened, clipped to [0, 1]."""
    bits = np.asarray(x0, dtype=np.float32).view(np.int32).astype(np.int64)
    w = (bits[:, None] + np.arange(-K, K + 1)[None]).reshape(-1)
    w = np.clip(w, 0, np.int64(np.float32(1.0).view(np.int32)))
    return w.astype(np.int32).view(np.float32)


def end_uniforms() -> np.ndarray:
    """u = 0, u = 1 - k * 2^-24 for k = 1..64, and u = 1 exactly."""
    return np.concatenate([[0.0], 1.0 - np.arange(1, 65) * 2.0 ** -24, [1.0]]).astype(np.float32)
