// MNN ("message neural network", gnn/mpnn.py:16-74) kernels of the HIP path (gfx950): the typed segmented sums
// of the aggregate-first message function and the plain graph sum of its readout.
//
// The reference forms, per edge i <- j with bond vector e, the [M, H] matrix sum_f e_f W[:, :, f] and multiplies it
// with h_j (an E x M x H temporary).  W is linear, so the sums can be formed first:
//   messages[i] = sum_f W_f . S_f[i],   S_f[i] = sum over the edges i <- j of type f of h_j
// With S stored as S[i, k * Fe + f] the messages are ONE plain GEMM on the parameter as PyTorch stores it:
// messages = S . W.view(M, H * Fe)^T (gi_gemm), and dW.view(M, H * Fe) = dMsg^T . S.
// Like seg_sum_kernel (gi_ops.hip): no atomics, every output summed in a fixed order (deterministic), index loads
// shared by the lanes of a row (broadcast), 16-byte row reads.
#include <stdlib.h>

#include "gi_common.h"

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

// bond type of message row u: rows are bond-type-major, type t = [type_off[t], type_off[t + 1])
template <int FE>
__device__ __forceinline__ int row_type(const int* __restrict__ type_off, int u) {
    int t = 0;
#pragma unroll
    for (int f = 1; f < FE; ++f) t += u >= type_off[f] ? 1 : 0;
    return t;
}

// S[c, k * FE + t] = sum over the dst-CSR slots s of row c whose message row has type t of h[u_src[in_perm[s]], k].
// One thread per (row, 4 hidden columns): it owns 4 * FE contiguous outputs (FE 16-byte stores when all 4 columns
// exist).  Rows without in-edges (row S among them) are written as 0.
template <int FE>
__global__ __launch_bounds__(256) void typed_seg_sum_kernel(
    const float* __restrict__ h, int ldh, const int* __restrict__ u_src, const int* __restrict__ in_perm,
    const int* __restrict__ seg_off, const int* __restrict__ type_off, int rows, int H, int c4n,
    float* __restrict__ out, int ldo, const int* __restrict__ rows_dev) {
    if (rows_dev) rows = min(rows, *rows_dev);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t / c4n), q = (int)(t - (long long)c * c4n);
    if (c >= rows) return;
    v4f acc[FE];
#pragma unroll
    for (int f = 0; f < FE; ++f) acc[f] = v4f{0.f, 0.f, 0.f, 0.f};
    const int lo = seg_off[c], hi = seg_off[c + 1];
    for (int s = lo; s < hi; ++s) {
        const int u = in_perm[s];
        const int ty = row_type<FE>(type_off, u);
        const v4f x = *(const v4f*)(h + (long long)u_src[u] * ldh + 4 * q);
#pragma unroll
        for (int f = 0; f < FE; ++f)
            if (f == ty) acc[f] += x;                 // (select, not a dynamic register index)
    }
    float* dst = out + (long long)c * ldo + (long long)4 * q * FE;
    if (4 * q + 4 <= H) {
        float v[4 * FE];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int f = 0; f < FE; ++f) v[j * FE + f] = acc[f][j];
#pragma unroll
        for (int i = 0; i < FE; ++i) *(v4f*)(dst + 4 * i) = v4f{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
    } else {
        for (int j = 0; j < 4 && 4 * q + j < H; ++j)
#pragma unroll
            for (int f = 0; f < FE; ++f) dst[j * FE + f] = acc[f][j];
    }
}

// Transpose (backward): dh[c, k] (+)= sum over the message rows u that row c sends (out_perm[src_off[c] ..)) of
// sum over u's edges (mu_off[u] ..) of dS[mu_dst[e], k * FE + type(u)].  One thread per (row, 4 hidden columns).
template <int FE>
__global__ __launch_bounds__(256) void typed_seg_sum_t_kernel(
    const float* __restrict__ dS, int lds, const int* __restrict__ out_perm, const int* __restrict__ src_off,
    const int* __restrict__ mu_off, const int* __restrict__ mu_dst, const int* __restrict__ type_off, int rows,
    int H, int c4n, float* __restrict__ dh, int lddh, int accumulate) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t / c4n), q = (int)(t - (long long)c * c4n);
    if (c >= rows) return;
    const int ncol = min(4, H - 4 * q);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int lo = src_off[c], hi = src_off[c + 1];
    for (int s = lo; s < hi; ++s) {
        const int u = out_perm[s];
        const int ty = row_type<FE>(type_off, u);
        const int e1 = mu_off[u + 1];
        for (int e = mu_off[u]; e < e1; ++e) {
            const float* src = dS + (long long)mu_dst[e] * lds + (long long)4 * q * FE + ty;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < ncol) acc[j] += src[j * FE];
        }
    }
    float* dst = dh + (long long)c * lddh + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < ncol) dst[j] = accumulate ? dst[j] + acc[j] : acc[j];
}

// g[b, k] = sum over the N slots of graph b of h[cidx[b * N + n], k] (padded slots read the zero row), stored to up to
// three destinations (GlobalReadout's fAddNet2 / fConnNet2 input tails and fTermNet2's input)
__global__ __launch_bounds__(256) void graph_sum_fwd_kernel(
    const float* __restrict__ h, int ldh, const int* __restrict__ cidx, int B, int N, int H, float* out0, int ld0,
    float* out1, int ld1, float* out2, int ld2) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = (int)(t / H), k = (int)(t - (long long)b * H);
    if (b >= B) return;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc += h[(long long)cidx[b * N + n] * ldh + k];
    if (out0) out0[(long long)b * ld0 + k] = acc;
    if (out1) out1[(long long)b * ld1 + k] = acc;
    if (out2) out2[(long long)b * ld2 + k] = acc;
}

// dh[c, k] (+)= dg0[b, k] + dg1[b, k] + dg2[b, k] with b the graph of compact row c (slot_of[c] / N), c < S;
// row S (the shared zero row of the padded slots) is set to 0 when not accumulating.
__global__ __launch_bounds__(256) void graph_sum_bwd_kernel(
    const float* __restrict__ dg0, int ld0, const float* __restrict__ dg1, int ld1, const float* __restrict__ dg2,
    int ld2, const int* __restrict__ slot_of, int S, int N, int H, float* __restrict__ dh, int lddh, int accumulate) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t / H), k = (int)(t - (long long)c * H);
    if (c > S) return;
    float* dst = dh + (long long)c * lddh + k;
    if (c == S) {
        if (!accumulate) *dst = 0.f;
        return;
    }
    const int b = slot_of[c] / N;
    float v = 0.f;
    if (dg0) v += dg0[(long long)b * ld0 + k];
    if (dg1) v += dg1[(long long)b * ld1 + k];
    if (dg2) v += dg2[(long long)b * ld2 + k];
    *dst = accumulate ? *dst + v : v;
}

}  // namespace

int gi_typed_seg_sum_n(const float* h, int ldh, const int* u_src, const int* in_perm, const int* seg_off,
                       const int* type_off, int rows, int H, int Fe, float* out, int ldo, const int* rows_dev,
                       void* stream) {
    (void)hipGetLastError();
    if (rows <= 0) return 0;
    if (!h || !seg_off || !type_off || !out || H <= 0 || Fe < 1 || Fe > GI_MAX_GROUPS || (ldh & 3) || ldh < gi_r4(H) ||
        ldo < H * Fe || (ldo & 3))
        return GI_EINVAL;
    if (((uintptr_t)h & 15) || ((uintptr_t)out & 15)) return GI_EINVAL;
    const int c4n = gi_cdiv(H, 4);
    const long long threads = (long long)rows * c4n;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    GiProfScope prof((hipStream_t)stream, GI_PROF_SEGSUM, 0.0);
#define GI_TSS(F) case F: hipLaunchKernelGGL(typed_seg_sum_kernel<F>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, \
                                             h, ldh, u_src, in_perm, seg_off, type_off, rows, H, c4n, out, ldo, rows_dev); break
    switch (Fe) { GI_TSS(1); GI_TSS(2); GI_TSS(3); GI_TSS(4); GI_TSS(5); GI_TSS(6); GI_TSS(7); GI_TSS(8); }
#undef GI_TSS
    return gi_launch_status();
}

extern "C" int gi_typed_seg_sum(const float* h, int ldh, const int* u_src, const int* in_perm, const int* seg_off,
                                const int* type_off, int rows, int H, int Fe, float* out, int ldo, void* stream) {
    return gi_typed_seg_sum_n(h, ldh, u_src, in_perm, seg_off, type_off, rows, H, Fe, out, ldo, nullptr, stream);
}

extern "C" int gi_typed_seg_sum_t(const float* dS, int lds, const int* out_perm, const int* src_off,
                                  const int* mu_off, const int* mu_dst, const int* type_off, int rows, int H, int Fe,
                                  float* dh, int lddh, int accumulate, void* stream) {
    (void)hipGetLastError();
    if (rows <= 0) return 0;
    if (!dS || !src_off || !type_off || !dh || H <= 0 || Fe < 1 || Fe > GI_MAX_GROUPS || lds < H * Fe || lddh < H)
        return GI_EINVAL;
    const int c4n = gi_cdiv(H, 4);
    const long long threads = (long long)rows * c4n;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    GiProfScope prof((hipStream_t)stream, GI_PROF_SEGSUM, 0.0);
#define GI_TST(F) case F: hipLaunchKernelGGL(typed_seg_sum_t_kernel<F>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, \
                                             dS, lds, out_perm, src_off, mu_off, mu_dst, type_off, rows, H, c4n, dh, lddh, \
                                             accumulate); break
    switch (Fe) { GI_TST(1); GI_TST(2); GI_TST(3); GI_TST(4); GI_TST(5); GI_TST(6); GI_TST(7); GI_TST(8); }
#undef GI_TST
    return gi_launch_status();
}

extern "C" int gi_graph_sum_fwd(const float* h, int ldh, const int* cidx, int B, int N, int H, float* out0, int ld0,
                                float* out1, int ld1, float* out2, int ld2, void* stream) {
    (void)hipGetLastError();
    if (B <= 0) return 0;
    if (!h || !cidx || N <= 0 || H <= 0 || ldh < H || (out0 && ld0 < H) || (out1 && ld1 < H) || (out2 && ld2 < H))
        return GI_EINVAL;
    const long long threads = (long long)B * H;
    hipLaunchKernelGGL(graph_sum_fwd_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, h, ldh, cidx, B, N, H, out0, ld0, out1, ld1, out2, ld2);
    return gi_launch_status();
}

extern "C" int gi_graph_sum_bwd(const float* dg0, int ld0, const float* dg1, int ld1, const float* dg2, int ld2,
                                const int* slot_of, int S, int N, int H, float* dh, int lddh, int accumulate,
                                void* stream) {
    (void)hipGetLastError();
    if (S < 0 || !dh || N <= 0 || H <= 0 || lddh < H || (S > 0 && !slot_of)) return GI_EINVAL;
    if ((dg0 && ld0 < H) || (dg1 && ld1 < H) || (dg2 && ld2 < H)) return GI_EINVAL;
    const long long threads = (long long)(S + 1) * H;
    hipLaunchKernelGGL(graph_sum_bwd_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, dg0, ld0, dg1, ld1, dg2, ld2, slot_of, S, N, H, dh, lddh, accumulate);
    return gi_launch_status();
}
