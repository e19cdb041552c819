// Log-likelihood of whole molecules along their decoding routes (gfx950): for route row r with logits z_r [W] and hot
// APD index a_r, row_ll[r] = z_r[a_r] - logsumexp(z_r), and mol_ll[m] = the sum of its rows' values — the log of the
// product over the route of the per-row probability of Analyzer.py:754-774 with a one-hot target, evaluated in log
// space with the row maximum subtracted (the reference's linear-space product underflows on long routes).
//
// Launches:
//   row_loglik_kernel      one wave per row, the row read ONCE: every lane keeps a running (max, sum of exp(z - max))
//                          over its share, the 64 pairs are merged by a butterfly.  16-byte loads over the aligned
//                          middle of the row, scalar loads for the head and tail, so any W and any row pitch run.
//   row_loglik_bwd_kernel  one wave per row: d_logits[r, j] = g_r (delta(j, a_r) - exp(z[r, j] - lse_r)), written
//                          (not accumulated), the probabilities renormalised by their own sum; g_r =
//                          g_mol[row_mol[r]] (+ g_kind[row_mol[r], kind_r]), or g_mol[r] when row_mol is NULL.
//   mol_check_kernel       the contract of the sum: row_mol in [-1, n_mol) and non-decreasing over the rows != -1
//   mol_sum_kernel         one thread per row; the thread of a molecule's FIRST row in the launch adds that molecule's
//                          rows to mol_ll[m] one by one in row order: one writer per molecule and launch, no atomics,
//                          so a route cut by a chunk boundary is continued by the next launch bit for bit as one
//                          sequential fp32 sum.
// Every loop is bounded by rows / W; hot and row_mol are range-checked before anything is indexed with them.
#include "gi_common.h"

#include <math.h>

namespace {

constexpr int ROWS_PER_BLOCK = 4;                          // one wave each

struct MaxSum { float m, s; };                        // s = sum_j exp(z_j - m) over the entries seen; (-inf, 0) = none

// exp(x - m) with m = -inf read as 0 (nothing seen yet: every x is -inf or NaN there; exp(-inf) = 0, exp(NaN) = NaN)
__device__ __forceinline__ float base_of(float m) { return m == -INFINITY ? 0.f : m; }

__device__ __forceinline__ void ms_add4(MaxSum& a, float v0, float v1, float v2, float v3) {
    const float m = fmaxf(fmaxf(a.m, fmaxf(v0, v1)), fmaxf(v2, v3));      // fmaxf drops NaNs: they enter through exp
    const float b = base_of(m);
    a.s = a.s * gi_exp_nonpos(a.m - b) + ((gi_exp_nonpos(v0 - b) + gi_exp_nonpos(v1 - b)) +
                                          (gi_exp_nonpos(v2 - b) + gi_exp_nonpos(v3 - b)));
    a.m = m;
}
__device__ __forceinline__ void ms_add1(MaxSum& a, float v) {
    const float m = fmaxf(a.m, v);
    const float b = base_of(m);
    a.s = a.s * gi_exp_nonpos(a.m - b) + gi_exp_nonpos(v - b);
    a.m = m;
}
__device__ __forceinline__ MaxSum ms_wave(MaxSum a) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const float om = __shfl_xor(a.m, sh), os = __shfl_xor(a.s, sh);
        const float m = fmaxf(a.m, om);
        const float b = base_of(m);
        a.s = a.s * gi_exp_nonpos(a.m - b) + os * gi_exp_nonpos(om - b);
        a.m = m;
    }
    return a;
}

// floats in front of the first 16-byte boundary of a row (a float pointer is 4-byte aligned), at most W
__device__ __forceinline__ int head_of(const float* p, int W) {
    const int h = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
    return h < W ? h : W;
}

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void row_loglik_kernel(const float* __restrict__ logits,
                                                                        long long ld, int rows, int W,
                                                                        const int* __restrict__ hot,
                                                                        float* __restrict__ row_ll,
                                                                        float* __restrict__ row_lse,
                                                                        int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int h = hot[r];
    if (h == -1) {                                        // a padding row: nothing is read
        if (lane == 0) { row_ll[r] = 0.f; row_lse[r] = 0.f; }
        return;
    }
    if (h < -1 || h >= W) {                               // nothing is indexed with it, nothing is written
        if (lane == 0) atomicOr(err, GI_LL_ERR_HOT);
        return;
    }
    const float* z = logits + (size_t)r * (size_t)ld;
    const int head = head_of(z, W);
    const int nvec = (W - head) >> 2;
    const int tail0 = head + 4 * nvec;                    // tail: [tail0, W), fewer than 4
    MaxSum a = {-INFINITY, 0.f};
    if (lane < head) ms_add1(a, z[lane]);
    const float4* zv = reinterpret_cast<const float4*>(z + head);
    for (int i = lane; i < nvec; i += 64) {
        const float4 v = zv[i];
        ms_add4(a, v.x, v.y, v.z, v.w);
    }
    if (lane < W - tail0) ms_add1(a, z[tail0 + lane]);
    a = ms_wave(a);
    if (lane == 0) {
        const float ls = logf(a.s);
        row_lse[r] = a.m + ls;
        row_ll[r] = (z[h] - a.m) - ls;                    // an all -inf row: NaN, as the fp64 expression gives
    }
}

__device__ __forceinline__ int kind_of(int h, int n_add, int n_conn) {
    return h < n_add ? 0 : h < n_add + n_conn ? 1 : 2;
}

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void row_loglik_bwd_kernel(
        const float* __restrict__ logits, long long ld, int rows, int W, const int* __restrict__ hot,
        const float* __restrict__ row_lse, const float* __restrict__ g_mol, const float* __restrict__ g_kind,
        const int* __restrict__ row_mol, int n_mol, int n_add, int n_conn, float* __restrict__ d_logits,
        long long ldd, int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* d = d_logits + (size_t)r * (size_t)ldd;
    const int h = hot[r];
    const int m = row_mol ? row_mol[r] : r;
    const bool bad_hot = h < -1 || h >= W, bad_mol = row_mol && (m < -1 || m >= n_mol);
    if (h == -1 || m == -1 || bad_hot || bad_mol) {       // an exactly zero row; nothing is read or indexed
        if ((bad_hot || bad_mol) && lane == 0) atomicOr(err, bad_hot ? GI_LL_ERR_HOT : GI_LL_ERR_MOL);
        for (int j = lane; j < W; j += 64) d[j] = 0.f;
        return;
    }
    float g = g_mol[m];
    if (g_kind) g += g_kind[(size_t)m * 3 + kind_of(h, n_add, n_conn)];
    const float* z = logits + (size_t)r * (size_t)ld;
    const float lse = row_lse[r];
    const int head = head_of(z, W);
    const int nvec = (W - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const float4* zv = reinterpret_cast<const float4*>(z + head);
    // row_lse is rounded at the LOGITS' magnitude (half an ulp of |lse| is a relative error of every probability: 4e-6
    // at |lse| = 100), so the probabilities are renormalised by their own sum; the second pass finds the row in cache
    float sum = 0.f;
    if (lane < head) sum += gi_exp_nonpos(z[lane] - lse);
    for (int i = lane; i < nvec; i += 64) {
        const float4 v = zv[i];
        sum += (gi_exp_nonpos(v.x - lse) + gi_exp_nonpos(v.y - lse)) +
               (gi_exp_nonpos(v.z - lse) + gi_exp_nonpos(v.w - lse));
    }
    if (lane < W - tail0) sum += gi_exp_nonpos(z[tail0 + lane] - lse);
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh);
    const float inv = 1.f / sum;
#define GI_LL_D(j_, z_) (g * (((j_) == h ? 1.f : 0.f) - gi_exp_nonpos((z_) - lse) * inv))
    if (head_of(d, W) != head) {                          // the two rows sit differently in their 16-byte pieces
        for (int j = lane; j < W; j += 64) d[j] = GI_LL_D(j, z[j]);
        return;
    }
    if (lane < head) d[lane] = GI_LL_D(lane, z[lane]);
    float4* dv = reinterpret_cast<float4*>(d + head);
    for (int i = lane; i < nvec; i += 64) {
        const float4 v = zv[i];
        const int j = head + 4 * i;
        dv[i] = make_float4(GI_LL_D(j, v.x), GI_LL_D(j + 1, v.y), GI_LL_D(j + 2, v.z), GI_LL_D(j + 3, v.w));
    }
    if (lane < W - tail0) d[tail0 + lane] = GI_LL_D(tail0 + lane, z[tail0 + lane]);
#undef GI_LL_D
}

// the last row before r whose row_mol is not -1, or -1 (bounded by r)
__device__ __forceinline__ int prev_live(const int* __restrict__ row_mol, int r) {
    for (int q = r - 1; q >= 0; --q)
        if (row_mol[q] != -1) return q;
    return -1;
}

__global__ __launch_bounds__(256) void mol_check_kernel(const int* __restrict__ row_mol, int rows, int n_mol,
                                                        int* __restrict__ err) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int m = row_mol[r];
    if (m == -1) return;
    if (m < -1 || m >= n_mol) { atomicOr(err, GI_LL_ERR_MOL); return; }
    const int q = prev_live(row_mol, r);
    if (q >= 0 && row_mol[q] > m) atomicOr(err, GI_LL_ERR_ORDER);
}

__global__ __launch_bounds__(256) void mol_sum_kernel(const float* __restrict__ row_ll,
                                                      const int* __restrict__ row_mol, const int* __restrict__ hot,
                                                      int rows, int n_mol, int n_add, int n_conn,
                                                      float* __restrict__ mol_ll, float* __restrict__ mol_kind,
                                                      const int* __restrict__ err) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    if (*err & (GI_LL_ERR_MOL | GI_LL_ERR_ORDER)) return; // the check before this launch, or an earlier call, refused
    const int m = row_mol[r];
    if (m < 0 || m >= n_mol) return;
    const int q = prev_live(row_mol, r);
    if (q >= 0 && row_mol[q] == m) return;                // not the molecule's first row of the launch
    float acc = mol_ll[m];
    float k[3] = {0.f, 0.f, 0.f};
    if (mol_kind)
        for (int c = 0; c < 3; ++c) k[c] = mol_kind[(size_t)m * 3 + c];
    for (int p = r; p < rows; ++p) {
        const int pm = row_mol[p];
        if (pm == -1) continue;
        if (pm != m) break;
        const float v = row_ll[p];
        acc += v;
        if (mol_kind) {
            const int h = hot[p];
            if (h >= 0) {
                const int c = kind_of(h, n_add, n_conn);
                k[0] += c == 0 ? v : 0.f;
                k[1] += c == 1 ? v : 0.f;
                k[2] += c == 2 ? v : 0.f;
            }
        }
    }
    mol_ll[m] = acc;
    if (mol_kind)
        for (int c = 0; c < 3; ++c) mol_kind[(size_t)m * 3 + c] = k[c];
}

bool kinds_ok(int W, int n_add, int n_conn) {
    return n_add >= 0 && n_conn >= 0 && (long long)n_add + n_conn + 1 == W;
}

}  // namespace

extern "C" int gi_row_loglik(const float* logits, long long ld, int rows, int W, const int* hot, float* row_ll,
                             float* row_lse, int* err, void* stream) {
    (void)hipGetLastError();
    if (rows < 0 || W < 1 || ld < W) return GI_EINVAL;
    if (rows == 0) return 0;
    if (!logits || !hot || !row_ll || !row_lse || !err) return GI_EINVAL;
    hipLaunchKernelGGL(row_loglik_kernel, dim3(gi_cdiv(rows, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0,
                       (hipStream_t)stream, logits, ld, rows, W, hot, row_ll, row_lse, err);
    return gi_launch_status();
}

extern "C" int gi_row_loglik_bwd(const float* logits, long long ld, int rows, int W, const int* hot,
                                 const float* row_lse, const float* g_mol, const float* g_kind, const int* row_mol,
                                 int n_mol, int n_add, int n_conn, float* d_logits, long long ldd, int* err,
                                 void* stream) {
    (void)hipGetLastError();
    if (rows < 0 || W < 1 || ld < W || ldd < W || n_mol < 0) return GI_EINVAL;
    if (rows == 0) return 0;
    if (!logits || !hot || !row_lse || !g_mol || !d_logits || !err) return GI_EINVAL;
    if (g_kind && (!row_mol || !kinds_ok(W, n_add, n_conn))) return GI_EINVAL;
    hipLaunchKernelGGL(row_loglik_bwd_kernel, dim3(gi_cdiv(rows, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0,
                       (hipStream_t)stream, logits, ld, rows, W, hot, row_lse, g_mol, g_kind, row_mol, n_mol, n_add,
                       n_conn, d_logits, ldd, err);
    return gi_launch_status();
}

extern "C" int gi_mol_loglik_sum(const float* row_ll, const int* row_mol, const int* hot, int rows, int n_mol, int W,
                                 int n_add, int n_conn, float* mol_ll, float* mol_kind, int* err, void* stream) {
    (void)hipGetLastError();
    if (rows < 0 || n_mol < 0) return GI_EINVAL;
    if (rows == 0 || n_mol == 0) return 0;
    if (!row_ll || !row_mol || !mol_ll || !err) return GI_EINVAL;
    if (mol_kind && (!hot || !kinds_ok(W, n_add, n_conn))) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mol_check_kernel, dim3(gi_cdiv(rows, 256)), dim3(256), 0, st, row_mol, rows, n_mol, err);
    hipLaunchKernelGGL(mol_sum_kernel, dim3(gi_cdiv(rows, 256)), dim3(256), 0, st, row_ll, row_mol, hot, rows, n_mol,
                       n_add, n_conn, mol_ll, mol_kind, (const int*)err);
    return gi_launch_status();
}
