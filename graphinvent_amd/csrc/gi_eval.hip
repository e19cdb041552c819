// Validation NLL of the "correct" actions (gfx950) — replaces the per-batch tensor work of
// `Analyzer.get_validation_likelihood` (Analyzer.py:754-774): softmax, target normalisation, product,
// row sum, `isnan` mask, `log`, the slice copy into the `likelihoods` buffer and the structure count.
// The boolean-mask index of the reference has a data-dependent length and so a host synchronisation
// per batch; here the compaction happens on the device and nothing is read back.
//
// Two launches per batch:
//   eval_row_kernel   one workgroup per row (the kl_loss_kernel pattern of gi_ops.hip): the row's
//                     correct-action probability s = sum_j (t_j / T) * softmax(o)_j in linear space, in
//                     the reference's per-element order, and target[b, W-1]
//   eval_scan_kernel  one workgroup: keep = !isnan(s), an order-preserving scan of the keep flags, the
//                     scatter of -log(s) to dst[start + rank], and the structure count summed in a fixed
//                     order.  A batch whose kept rows would run past dst writes nothing and sets *err
//                     (the reference raises on the shape mismatch before it writes or counts anything);
//                     once *err is set, later batches change nothing either.
// Deterministic: no atomics, every sum in a fixed order for a given B.
#include "gi_common.h"

namespace {

constexpr int SCAN_NT = 1024;

template <int NT>
__device__ __forceinline__ float eval_block_reduce(float x, bool is_max, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float y = __shfl_xor(x, s);
        x = is_max ? fmaxf(x, y) : x + y;
    }
    __syncthreads();
    if (lane == 0) red[wid] = x;
    __syncthreads();
    float r = red[0];                                          // the waves' partials in order
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// s[b] = sum_j (t_j / T) * (exp(o_j - max o) / sum_k exp(o_k - max o)),  last[b] = t[b, W-1].
// NaN when T == 0 (0 / 0) and when the row holds a NaN or +inf logit (the sum of exponentials is NaN);
// 0 when every correct action's probability underflows.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void eval_row_kernel(const float* __restrict__ out, int ldo,
                                                      const T* __restrict__ tgt, int ldt, int width,
                                                      float* __restrict__ s_out,
                                                      float* __restrict__ last_out) {
    __shared__ float red[NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* o = out + (long long)b * ldo;
    const T* t = tgt + (long long)b * ldt;
    float mx = -INFINITY, ts = 0.f;
    for (int j = tid; j < width; j += NT) { mx = fmaxf(mx, o[j]); ts += (float)t[j]; }
    mx = eval_block_reduce<NT>(mx, true, red);
    ts = eval_block_reduce<NT>(ts, false, red);
    float se = 0.f;
    for (int j = tid; j < width; j += NT) se += expf(o[j] - mx);
    se = eval_block_reduce<NT>(se, false, red);
    float s = 0.f;
    for (int j = tid; j < width; j += NT) {
        const float p = expf(o[j] - mx) / se;
        s += ((float)t[j] / ts) * p;
    }
    s = eval_block_reduce<NT>(s, false, red);
    if (tid == 0) {
        s_out[b] = s;
        last_out[b] = (float)t[width - 1];
    }
}

// One workgroup: rows in chunks of SCAN_NT; a wave's ranks from a ballot, the waves' offsets from LDS.
// Pass 1 counts the kept rows (and the structures), pass 2 scatters when the batch fits.
__global__ __launch_bounds__(SCAN_NT) void eval_scan_kernel(const float* __restrict__ s_in,
                                                            const float* __restrict__ last, int B,
                                                            float* __restrict__ dst, long long dst_len,
                                                            long long start,
                                                            float* __restrict__ n_structures,
                                                            int* __restrict__ err) {
    constexpr int NW = SCAN_NT / 64;
    __shared__ int wcount[NW];
    __shared__ float wsum[NW];
    __shared__ int total_sh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (*err) return;                                    // a previous batch overflowed: nothing more
    int kept = 0;
    float ns = 0.f;
    for (int b = tid; b < B; b += SCAN_NT) {
        kept += !__builtin_isnan(s_in[b]);
        ns += last[b];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        kept += __shfl_xor(kept, s);
        ns += __shfl_xor(ns, s);
    }
    if (lane == 0) { wcount[wid] = kept; wsum[wid] = ns; }
    __syncthreads();
    if (tid == 0) {
        int k = 0;
        float n = 0.f;
        for (int i = 0; i < NW; ++i) { k += wcount[i]; n += wsum[i]; }
        const bool fits = k == 0 || (start >= 0 && start + k <= dst_len);
        total_sh = fits ? k : -1;
        if (fits) n_structures[0] += n;
        else *err = 1;
    }
    __syncthreads();
    if (total_sh <= 0) return;
    int base = 0;                                         // kept rows of the previous chunks
    for (int c = 0; c < B; c += SCAN_NT) {
        const int b = c + tid;
        const float s = b < B ? s_in[b] : __builtin_nanf("");
        const bool keep = !__builtin_isnan(s);
        const unsigned long long m = __ballot(keep);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                                  // the previous chunk's wcount reads are done
        if (lane == 0) wcount[wid] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int i = 0; i < wid; ++i) off += wcount[i];
        if (keep) dst[start + off + rank] = -logf(s);
        for (int i = 0; i < NW; ++i) base += wcount[i];
    }
}

}  // namespace

extern "C" int gi_eval_nll(const float* out, int ldo, const void* target, int tgt_dtype, int ldt, int B,
                           int width, float* dst, long long dst_len, long long start, float* n_structures,
                           int* err, float* ws, void* stream) {
    (void)hipGetLastError();
    if (B <= 0) return 0;
    if (!out || !target || !dst || !n_structures || !err || !ws || width <= 0 || ldo < width ||
        ldt < width || dst_len < 0 || start < 0)
        return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    float* s = ws;                                        // ws: 2 B floats (s | last)
    float* last = ws + B;
    // rows wider than 2048 logits (ZINC / ChEMBL shapes) get 1024 threads each, as gi_kl_loss
#define GI_EVAL_LAUNCH(T_, NT_)                                                                   \
    hipLaunchKernelGGL((eval_row_kernel<T_, NT_>), dim3(B), dim3(NT_), 0, st, out, ldo,           \
                       (const T_*)target, ldt, width, s, last)
    if (tgt_dtype == GI_DTYPE_F32) {
        if (width > 2048) GI_EVAL_LAUNCH(float, 1024); else GI_EVAL_LAUNCH(float, 256);
    } else if (tgt_dtype == GI_DTYPE_I8) {
        if (width > 2048) GI_EVAL_LAUNCH(signed char, 1024); else GI_EVAL_LAUNCH(signed char, 256);
    }
#undef GI_EVAL_LAUNCH
    else
        return GI_EINVAL;
    hipLaunchKernelGGL(eval_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, s, last, B, dst, dst_len, start,
                       n_structures, err);
    return gi_launch_status();
}
