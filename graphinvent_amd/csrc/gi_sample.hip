// Sampling step of graph generation (gfx950): softmax of the APD logits, one categorical draw per
// graph, action decode and the validity rules — replaces `softmax(self.model(...))` +
// `GraphGenerator.get_actions` / `get_invalid_actions` (GraphGenerator.py:121, 467-657): a
// Multinomial object, a [B, W] one-hot sample, three `nonzero`s, boolean-mask gathers and ~15 small
// index kernels per generation step become ONE launch, one workgroup per graph.
//
// The draw is the inverse CDF of a caller-supplied uniform per graph (torch's Multinomial stream is
// not reproducible by any other implementation; the distribution is the same): the first action
// whose cumulative un-normalised probability exceeds u * total.  Cumulative sums run in a fixed
// order (256 contiguous chunks, sequential inside a chunk), so a (logits, u) pair always gives the
// same action.  HBM-bound: reads B*W*4 bytes once; the row lives in LDS between the passes.
//
// The claim rule is one fp32 cumulative function, monotone in the index, with no gaps at the chunk
// seams.  The running maximum of the inclusive scan of the chunk sums, clamped to the total, gives
// non-decreasing boundaries B(t) with B(255) = total, and chunk t owns the targets in [B(t-1), B(t));
// the last chunk also owns everything at or past the total (u = 1 included).  Inside its range the chunk
// walks from B(t-1) and takes the first element whose running sum exceeds the target.  When its walk
// ends below B(t) (fp32 rounding), or the target is at or past the total, it takes the last element
// with e > 0 at or before its end.  Only elements with e > 0 can be drawn.
#include "gi_common.h"

namespace {

constexpr int SAMPLE_MAX_W = 15360;        // floats of one APD row kept in LDS (60 KB)

// RL variant (GraphGeneratorRL.get_actions, GraphGeneratorRL.py:521-633): the draw from the agent's row
// is the same code path as above, bit for bit; the prior's row is streamed once (online maximum and
// rescaled sum, never kept in LDS) and read at the drawn index.  Saved for the backward: the flat
// index and the log-sum-exp of both rows.
struct RlOut {
    const float* prior;
    int ldp;
    int vec_agent, vec_prior;                // 16-byte aligned rows with a pitch % 4 == 0: float4 loads
    float* like_prior;
    int* idx;
    float* lse;                              // [B, 2]: agent, prior
};

// online softmax state: (m, s) = (running maximum, sum of exp(v - m))
__device__ __forceinline__ void osm_add(float& m, float& s, float v) {
    if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
    else if (v != -INFINITY) s += expf(v - m);
}

__device__ __forceinline__ void osm_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;
    s = (s > 0.f ? s * expf(m - M) : 0.f) + (s2 > 0.f ? s2 * expf(m2 - M) : 0.f);
    m = M;
}

template <typename ET, bool RL>
__global__ __launch_bounds__(256) void sample_actions_kernel(
    const float* __restrict__ logits, int ldl, const float* __restrict__ uniform,
    const int* __restrict__ n_nodes, const ET* __restrict__ edges, int N, int A, int Fe,
    int* __restrict__ action, float* __restrict__ likelihood, int* __restrict__ flags, RlOut rl) {
    __shared__ float e[SAMPLE_MAX_W];
    __shared__ float red[256];
    __shared__ float wtot[4], wmax[4];
    __shared__ int found_s;
    __shared__ int lastpos[256];             // per chunk: its last index with e > 0, or -1
    __shared__ float pm_s[4], ps_s[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int NA = N * A, NC = N * Fe, W = NA + NC + 1;
    const float* row = logits + (long long)b * ldl;
    // pass 1: row -> LDS, maximum (a maximum does not depend on the order: float4 loads change nothing)
    float mx = -INFINITY;
    if (RL && rl.vec_agent) {
        const float4* row4 = reinterpret_cast<const float4*>(row);
        for (int i = tid; i < W / 4; i += 256) {
            const float4 v = row4[i];
            e[4 * i] = v.x; e[4 * i + 1] = v.y; e[4 * i + 2] = v.z; e[4 * i + 3] = v.w;
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
        for (int i = (W & ~3) + tid; i < W; i += 256) {
            const float v = row[i];
            e[i] = v;
            mx = fmaxf(mx, v);
        }
    } else {
        for (int i = tid; i < W; i += 256) {
            const float v = row[i];
            e[i] = v;
            mx = fmaxf(mx, v);
        }
    }
    if constexpr (RL) {
        // the prior's row: one streamed pass, per-thread online softmax, then wave and block merges
        const float* prow = rl.prior + (long long)b * rl.ldp;
        float pm = -INFINITY, ps = 0.f;
        if (rl.vec_prior) {
            const float4* prow4 = reinterpret_cast<const float4*>(prow);
            for (int i = tid; i < W / 4; i += 256) {
                const float4 v = prow4[i];
                osm_add(pm, ps, v.x); osm_add(pm, ps, v.y); osm_add(pm, ps, v.z); osm_add(pm, ps, v.w);
            }
            for (int i = (W & ~3) + tid; i < W; i += 256) osm_add(pm, ps, prow[i]);
        } else {
            for (int i = tid; i < W; i += 256) osm_add(pm, ps, prow[i]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(pm, o), s2 = __shfl_xor(ps, o);
            osm_merge(pm, ps, m2, s2);
        }
        if (lane == 0) { pm_s[wid] = pm; ps_s[wid] = ps; }
    }
    red[tid] = mx;
    if (tid == 0) found_s = 0x7fffffff;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    // pass 2: un-normalised probabilities; sums of 256 contiguous chunks
    for (int i = tid; i < W; i += 256) e[i] = expf(e[i] - mx);
    __syncthreads();
    const int L = (W + 255) / 256;
    const int lo = min(tid * L, W), hi = min(lo + L, W);
    float csum = 0.f;
    int lp = -1;
    for (int i = lo; i < hi; ++i) {
        csum += e[i];
        if (e[i] > 0.f) lp = i;
    }
    lastpos[tid] = lp;
    // inclusive scan of the chunk sums in chunk order (wave shuffle + 4 wave totals): woff + x.  Its
    // intermediate window sums are not monotone, so neither is woff + x after a chunk of zeros: the
    // boundaries are its running maximum B(t), clamped to the total.  fl(woff + max x) = max fl(woff + x),
    // so the maximum is taken per wave on x and across waves on woff + wave maximum: exact.
    float x = csum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    float xm = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(xm, o);
        if (lane >= o) xm = fmaxf(xm, y);
    }
    const float xmprev = __shfl_up(xm, 1);
    if (lane == 63) { wtot[wid] = x; wmax[wid] = xm; }
    __syncthreads();
    float woff = 0.f, carry = 0.f;                   // carry: B of the previous wave's last chunk
    for (int w = 0; w < wid; ++w) {
        carry = fmaxf(carry, woff + wmax[w]);
        woff += wtot[w];
    }
    const float total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    // B(t-1) is the very value chunk t-1 computed as its B(t)
    const float bprev = lane ? fminf(fmaxf(carry, woff + xmprev), total) : fminf(carry, total);
    const float bend = fminf(fmaxf(carry, woff + xm), total);
    const float target = uniform[b] * total;
    // exactly one chunk owns any target >= 0 (a NaN target is owned by none: see the fallback below)
    if (bprev <= target && (target < bend || tid == 255)) {
        int k = -1;
        if (target < bend) {
            float c = bprev;
            for (int i = lo; i < hi; ++i) {
                c += e[i];                           // c > target >= c - e[i] only if e[i] > 0
                if (c > target) { k = i; break; }
            }
        }
        for (int t = tid; k < 0 && t >= 0; --t) k = lastpos[t];
        if (k >= 0) found_s = k;
    }
    __syncthreads();
    if (tid != 0) return;
    // the only ways to leave no claim are a NaN target (NaN or +inf logits) or a row with no e > 0:
    // both fall back to the last action
    int idx = found_s;
    if (idx >= W) idx = W - 1;
    const int nn = n_nodes[b];
    int kind, node = 0, rem = 0, from = 0, invalid = 0, reset = 0;
    if (idx < NA) {                                  // "add" (GraphGenerator.py:555-557)
        kind = 0; node = idx / A; rem = idx - node * A; from = nn;
        const bool empty = nn == 0;
        if (!empty && node >= nn) invalid = 1;       // :605-608 attach to a non-existing node
        if (empty && node != 0) invalid = 1;         // :611-614 first atom must go to slot 0
        if (from >= N) { invalid = 1; reset = 1; }   // :617 graph is full
        if (empty) reset = 1;                        // :650-654
        if (reset) from = 0;                         // :567
    } else if (idx < NA + NC) {                      // "connect" (:559-561)
        kind = 1;
        const int r = idx - NA;
        node = r / Fe; rem = r - node * Fe; from = nn - 1;
        if (node >= nn) invalid = 1;                 // :620
        if (nn == 0) invalid = 1;                    // :623
        if (node == from) invalid = 1;               // :626 self-loop
        const int fj = from < 0 ? from + N : from;   // torch indexing wraps -1 (:629-633)
        float adj = 0.f;
        const ET* ep = edges + (((long long)b * N + node) * N + fj) * Fe;
        for (int f = 0; f < Fe; ++f) adj += (float)ep[f];
        if (adj == 1.f) invalid = 1;                 // :629-633 bond already there
    } else {
        kind = 2;                                    // "terminate"
    }
    action[4 * b + 0] = kind; action[4 * b + 1] = node; action[4 * b + 2] = rem; action[4 * b + 3] = from;
    likelihood[b] = e[idx] / total;                  // :541 apds[one_hot == 1]
    flags[b] = invalid | (reset << 1);
    if constexpr (RL) {                              // GraphGeneratorRL.py:607-608 prior_apds[one_hot == 1]
        float pm = pm_s[0], ps = ps_s[0];
        for (int w = 1; w < 4; ++w) osm_merge(pm, ps, pm_s[w], ps_s[w]);
        rl.like_prior[b] = expf(rl.prior[(long long)b * rl.ldp + idx] - pm) / ps;
        rl.idx[b] = idx;
        rl.lse[2 * b + 0] = mx + logf(total);
        rl.lse[2 * b + 1] = pm + logf(ps);
    }
}

// d_logits[b, j] = g[b] * like[b] * (delta(j, idx[b]) - exp(l[b, j] - lse[b])): the Jacobian of
// softmax(l[b])[idx[b]] applied to the upstream gradient.  blockIdx.x = row * chunks + chunk,
// blockIdx.z = side (0 agent, 1 prior); 1024 columns per block.
struct LikeBwdSide {
    const float* logits;
    int ldl;
    const float* g;                          // NULL: this side is skipped
    const float* like;
    float* d;
    int ldd;
    int vec;                                 // float4 loads and stores allowed
};

constexpr int LBWD_COLS = 1024;

__global__ __launch_bounds__(256) void likelihood_bwd_kernel(LikeBwdSide s0, LikeBwdSide s1,
                                                             const int* __restrict__ idx,
                                                             const float* __restrict__ lse, int W,
                                                             int chunks) {
    const LikeBwdSide& s = blockIdx.z ? s1 : s0;
    if (!s.g) return;
    const int b = blockIdx.x / chunks, c0 = (blockIdx.x - b * chunks) * LBWD_COLS;
    const float gl = s.g[b] * s.like[b], L = lse[2 * b + blockIdx.z];
    const int k = idx[b];
    const float* row = s.logits + (long long)b * s.ldl;
    float* out = s.d + (long long)b * s.ldd;
    if (s.vec) {
        const int j = c0 + 4 * threadIdx.x;
        if (j + 3 < W) {
            const float4 v = *reinterpret_cast<const float4*>(row + j);
            float4 r;
            r.x = gl * ((j == k ? 1.f : 0.f) - expf(v.x - L));
            r.y = gl * ((j + 1 == k ? 1.f : 0.f) - expf(v.y - L));
            r.z = gl * ((j + 2 == k ? 1.f : 0.f) - expf(v.z - L));
            r.w = gl * ((j + 3 == k ? 1.f : 0.f) - expf(v.w - L));
            *reinterpret_cast<float4*>(out + j) = r;
        } else {
            for (int jj = j; jj < W; ++jj) out[jj] = gl * ((jj == k ? 1.f : 0.f) - expf(row[jj] - L));
        }
    } else {
#pragma unroll
        for (int q = 0; q < LBWD_COLS / 256; ++q) {
            const int j = c0 + q * 256 + threadIdx.x;
            if (j < W) out[j] = gl * ((j == k ? 1.f : 0.f) - expf(row[j] - L));
        }
    }
}

bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

}  // namespace

extern "C" int gi_sample_actions(const float* logits, int ldl, const float* uniform,
                                 const int* n_nodes, const void* edges, int edges_dtype, int B,
                                 int N, int A, int Fe, int* action, float* likelihood, int* flags,
                                 void* stream) {
    (void)hipGetLastError();   // drop stale errors of earlier, unrelated runtime calls
    if (B <= 0) return 0;
    if (!logits || !uniform || !n_nodes || !edges || !action || !likelihood || !flags || N <= 0 ||
        A <= 0 || Fe <= 0)
        return GI_EINVAL;
    const long long W = (long long)N * A + (long long)N * Fe + 1;
    if (W > SAMPLE_MAX_W) return GI_ELIMIT;
    if (ldl < W) return GI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const RlOut none{};
    if (edges_dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL((sample_actions_kernel<float, false>), dim3(B), dim3(256), 0, st, logits,
                           ldl, uniform, n_nodes, (const float*)edges, N, A, Fe, action, likelihood,
                           flags, none);
    else if (edges_dtype == GI_DTYPE_I8)
        hipLaunchKernelGGL((sample_actions_kernel<signed char, false>), dim3(B), dim3(256), 0, st,
                           logits, ldl, uniform, n_nodes, (const signed char*)edges, N, A, Fe, action,
                           likelihood, flags, none);
    else
        return GI_EINVAL;
    return gi_launch_status();
}

extern "C" int gi_sample_actions_rl(const float* agent_logits, int lda, const float* prior_logits,
                                    int ldp, const float* uniform, const int* n_nodes,
                                    const void* edges, int edges_dtype, int B, int N, int A, int Fe,
                                    int* action, float* like_agent, float* like_prior, int* flags,
                                    int* idx, float* lse, void* stream) {
    (void)hipGetLastError();
    if (B <= 0) return 0;
    if (!agent_logits || !prior_logits || !uniform || !n_nodes || !edges || !action ||
        !like_agent || !like_prior || !flags || !idx || !lse || N <= 0 || A <= 0 || Fe <= 0)
        return GI_EINVAL;
    const long long W = (long long)N * A + (long long)N * Fe + 1;
    if (W > SAMPLE_MAX_W) return GI_ELIMIT;
    if (lda < W || ldp < W) return GI_EINVAL;
    RlOut rl;
    rl.prior = prior_logits;
    rl.ldp = ldp;
    rl.vec_agent = (lda % 4 == 0) && aligned16(agent_logits);
    rl.vec_prior = (ldp % 4 == 0) && aligned16(prior_logits);
    rl.like_prior = like_prior;
    rl.idx = idx;
    rl.lse = lse;
    hipStream_t st = (hipStream_t)stream;
    if (edges_dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL((sample_actions_kernel<float, true>), dim3(B), dim3(256), 0, st,
                           agent_logits, lda, uniform, n_nodes, (const float*)edges, N, A, Fe,
                           action, like_agent, flags, rl);
    else if (edges_dtype == GI_DTYPE_I8)
        hipLaunchKernelGGL((sample_actions_kernel<signed char, true>), dim3(B), dim3(256), 0, st,
                           agent_logits, lda, uniform, n_nodes, (const signed char*)edges, N, A, Fe,
                           action, like_agent, flags, rl);
    else
        return GI_EINVAL;
    return gi_launch_status();
}

extern "C" int gi_sample_likelihood_bwd(int B, int W, const int* idx, const float* lse,
                                        const float* agent_logits, int lda, const float* g_agent,
                                        const float* like_agent, float* d_agent, int ldda,
                                        const float* prior_logits, int ldp, const float* g_prior,
                                        const float* like_prior, float* d_prior, int lddp,
                                        void* stream) {
    (void)hipGetLastError();
    if (B <= 0 || (!g_agent && !g_prior)) return 0;
    if (W <= 0 || !idx || !lse) return GI_EINVAL;
    if (W > SAMPLE_MAX_W) return GI_ELIMIT;
    if (g_agent && (!agent_logits || !like_agent || !d_agent || lda < W || ldda < W)) return GI_EINVAL;
    if (g_prior && (!prior_logits || !like_prior || !d_prior || ldp < W || lddp < W)) return GI_EINVAL;
    const LikeBwdSide s0{agent_logits, lda, g_agent, like_agent, d_agent, ldda,
                         lda % 4 == 0 && ldda % 4 == 0 && aligned16(agent_logits) && aligned16(d_agent)};
    const LikeBwdSide s1{prior_logits, ldp, g_prior, like_prior, d_prior, lddp,
                         ldp % 4 == 0 && lddp % 4 == 0 && aligned16(prior_logits) && aligned16(d_prior)};
    const int chunks = (W + LBWD_COLS - 1) / LBWD_COLS;
    if ((long long)B * chunks > 0x7fffffffLL) return GI_ELIMIT;
    hipLaunchKernelGGL(likelihood_bwd_kernel, dim3(B * chunks, 1, 2), dim3(256), 0,
                       (hipStream_t)stream, s0, s1, idx, lse, W, chunks);
    return gi_launch_status();
}
