// fp16x2 forward / dgrad GEMM of the node-level hidden layers (gfx950): bias + SELU or * selu'(act) epilogues.
//
//   C[M, N] = epilogue( A[M, K] . B[N, K]^T ),  A and B plain fp32 with k contiguous (GI_GEMM_BF3B_F32 | GI_GEMM_X2)
//
// The arithmetic is gi_gemm_bf3_kernel's fp16x2 form, bit for bit: the same per-tensor scales (gx_scale), the same
// split (gx_split2), every accumulator fed ascending 16-deep k blocks with the terms a2 b1, a1 b2, a1 b1 on
// v_mfma_f32_32x32x16_f16, the same zero fill past K and the same epilogue expressions.  What differs is the data flow:
//   - the four waves split the 128 x 128 block tile by COLUMNS (1 x 4 waves, wave tile 128 x 32): a wave's B columns
//     are its own, so B goes global -> registers -> split -> MFMA operand and never touches LDS.  Only A (shared by
//     all four waves) is staged, as two fp16 planes: half the LDS stores of the 2 x 2 layout at the same LDS reads.
//   - 32-deep k steps (two 16-deep blocks), one barrier per step; A travels as ds_write_b128 (8 k per thread and
//     plane); 32 KB of LDS per workgroup, <= 168 VGPRs -> three workgroups per CU.
//   - the tile order is a stream over the REAL row tiles (m_dev read on the device): groups of a row panel's column
//     tiles go round-robin to the 8 XCDs (workgroup b runs on XCD b & 7), so the tiles that share an A row panel
//     share one L2; every XCD gets its share of each problem, the widest problems first.
// Side effects as the kernel it replaces: c_amax gets, slot for slot, the maxima the 2 x 2 kernel published (each
// wave's half quadrants go to the slot of the 64 x 64 quadrant they belong to), and the dynamic-range guard counts
// the low rows of the first column tile once per row.
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <type_traits>

#include "gi_common.h"
#include "gi_gemm_plan.h"
#include "gi_mfma.h"
#include "gi_x2.h"

typedef unsigned xn_u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int XN_BM = 128, XN_BN = 128, XN_BK = 32;           // block tile; k step = two 16-deep MFMA blocks
constexpr int XN_ROWB = 32;                                   // bytes of one row of one plane of a 16-deep block
constexpr int XN_PLANE = 128 * XN_ROWB;                       // 4 KB
constexpr int XN_SUB = 2 * XN_PLANE + 64;                     // one 16-deep block (two planes); +64: the four k chunks
                                                              // a row's writers store hit distinct banks
constexpr int XN_BUF = 2 * XN_SUB;                            // one 32-deep step

__host__ __device__ inline int xn_r32(int k) { return (k + 31) & ~31; }

// m_end of problem i (device)
__device__ __forceinline__ int xn_m_end(const gi_gemm_params& p) { return p.m_dev ? max(min(p.M, *p.m_dev), 0) : p.M; }

// EPI: 1 = bias + SELU (forward), 2 = * selu'(act) (dgrad)
template <int EPI>
__global__ __launch_bounds__(256, 3) void gi_gemm_x2n_kernel(const GiGemmBatch b) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XN_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;

    // ---- tile: stream over the real row tiles, a row panel's column tiles on one XCD (block-uniform) ----------
    int pi = -1, by = 0, bx = 0;
    {
        const int x = blockIdx.x & 7;
        int j = blockIdx.x >> 3, g0 = 0;                          // g0: first row panel (group) of problem i
        for (int i = 0; i < b.n; ++i) {
            const int rows = (xn_m_end(b.p[i]) + XN_BM - 1) / XN_BM, gx = b.gx[i];
            const int first = g0 + (((x - g0) % 8) + 8) % 8;      // first group of this XCD in [g0, g0 + rows)
            const int cnt = first < g0 + rows ? (g0 + rows - 1 - first) / 8 + 1 : 0;
            if (j < cnt * gx) {
                const int gi = j / gx;
                pi = i; bx = j - gi * gx; by = first + 8 * gi - g0;
                break;
            }
            j -= cnt * gx;
            g0 += rows;
        }
    }
    if (pi < 0) return;                                          // beyond this XCD's share of the real tiles
    const gi_gemm_params& p = b.p[pi];
    const int m_end = xn_m_end(p);
    const int m0 = by * XN_BM, n0 = bx * XN_BN;
    const int K = p.K, ns = xn_r32(K) / XN_BK;                    // 32-deep steps: the 16-deep blocks of Kp = r32(K)
    float sa, ia, sb, ib;                                        // per-tensor power-of-two scales
    gx_scale(gx_amax_read(p.a_amax), sa, ia);
    gx_scale(gx_amax_read(p.b_amax), sb, ib);

    // ---- staging coordinates ---------------------------------------------------------------------------------
    // A: 128 rows x 4 chunks of 8 k per step -> 2 chunks per thread: chunk c8 = tid & 3 (16-deep block c8 >> 1, its
    // 16-byte half c8 & 1), rows (tid >> 2) + 64 i
    const int c8 = tid & 3;
    unsigned a_off[2], a_lds[2];
    const int a_cmax = (p.lda >= ((K + 3) & ~3)) ? ((K + 3) & ~3) - 4 : K - 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int rl = (tid >> 2) + 64 * i;
        const int row = min(m0 + rl, m_end - 1);
        a_off[i] = (unsigned)row * (unsigned)p.lda * 4u;
        a_lds[i] = (c8 >> 1) * XN_SUB + rl * XN_ROWB + 16 * ((c8 & 1) ^ ((rl >> 3) & 1));
    }
    // B: lane (l31, lhi) of wave wid holds column n0 + 32 wid + l31, k 8 lhi .. 8 lhi + 7 of each 16-deep block — the
    // MFMA's B-operand layout, loaded straight from the row
    const int bcol = min(n0 + 32 * wid + l31, p.N - 1);
    const unsigned b_off = (unsigned)bcol * (unsigned)p.ldb * 4u;
    const int b_cmax = (p.ldb >= ((K + 3) & ~3)) ? ((K + 3) & ~3) - 4 : K - 4;

    float rowmax[2] = {0.f, 0.f};                                // fp16x2 guard: largest |A| of this thread's two rows
    v4f ra[2][2], rb[2][2];                                      // the next step in flight: [row | block][half]
    xn_u32x4 bh[2][2];                                           // B planes of the current step: [block][plane]

    auto gload = [&](auto steady_c, int kt) __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady_c)::value;
        const int k0 = kt * XN_BK;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ka = k0 + 8 * c8 + 4 * h;
                if (STEADY) ra[i][h] = *(const v4f_u*)((const char*)p.A + a_off[i] + 4u * (unsigned)ka);
                else ra[i][h] = gi_load4_raw((const float*)((const char*)p.A + a_off[i]), ka, a_cmax);
            }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kb = k0 + 16 * s + 8 * lhi + 4 * h;
                if (STEADY) rb[s][h] = *(const v4f_u*)((const char*)p.B + b_off + 4u * (unsigned)kb);
                else rb[s][h] = gi_load4_raw((const float*)((const char*)p.B + b_off), kb, b_cmax);
            }
    };
    // split the step in flight: A -> LDS buffer buf, B -> bh
    auto split = [&](auto steady_c, int kt, int buf) __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady_c)::value;
        const int k0 = kt * XN_BK;
        unsigned char* As = smem + buf * XN_BUF;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xn_u32x4 w0, w1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v4f v = ra[i][h];
                if (!STEADY) v = gi_fix4(v, k0 + 8 * c8 + 4 * h, a_cmax, K, true);
                rowmax[i] = fmaxf(fmaxf(rowmax[i], fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
                unsigned x0, x1, y0, y1;
                gx_split2(v.x, v.y, sa, x0, x1);
                gx_split2(v.z, v.w, sa, y0, y1);
                w0[2 * h] = x0; w0[2 * h + 1] = y0; w1[2 * h] = x1; w1[2 * h + 1] = y1;
            }
            *reinterpret_cast<xn_u32x4*>(As + a_lds[i]) = w0;
            *reinterpret_cast<xn_u32x4*>(As + XN_PLANE + a_lds[i]) = w1;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v4f v = rb[s][h];
                if (!STEADY) v = gi_fix4(v, k0 + 16 * s + 8 * lhi + 4 * h, b_cmax, K, true);
                unsigned x0, x1, y0, y1;
                gx_split2(v.x, v.y, sb, x0, x1);
                gx_split2(v.z, v.w, sb, y0, y1);
                bh[s][0][2 * h] = x0; bh[s][0][2 * h + 1] = y0; bh[s][1][2 * h] = x1; bh[s][1][2 * h + 1] = y1;
            }
    };

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    auto compute = [&](int buf) __attribute__((always_inline)) {
        const unsigned char* As = smem + buf * XN_BUF;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int r = t * 32 + l31;
                const int oa = s * XN_SUB + r * XN_ROWB + 16 * (lhi ^ ((r >> 3) & 1));
                const gx_f16x8 a1 = *reinterpret_cast<const gx_f16x8*>(As + oa);
                const gx_f16x8 a2 = *reinterpret_cast<const gx_f16x8*>(As + XN_PLANE + oa);
                // a2 b1 + a1 b2 + a1 b1 (smallest terms first), as gi_gemm_bf3_kernel: one accumulator's chain at a time
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, __builtin_bit_cast(gx_f16x8, bh[s][0]), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, __builtin_bit_cast(gx_f16x8, bh[s][1]), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, __builtin_bit_cast(gx_f16x8, bh[s][0]), acc[t], 0, 0, 0);
            }
    };

    // ---- k loop: the next step's loads in flight under this step's MFMAs, one barrier per step ------------------
    const std::true_type ST{};
    const std::false_type GEN{};
    const int n_full = K / XN_BK;                                // steps that are full in k
    if (n_full > 0) { gload(ST, 0); split(ST, 0, 0); } else { gload(GEN, 0); split(GEN, 0, 0); }
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < n_full; ++kt) {                              // step kt + 1 is full
        gload(ST, kt + 1);
        compute(kt & 1);
        split(ST, kt + 1, (kt + 1) & 1);
        __syncthreads();
    }
    for (; kt < ns; ++kt) {                                      // the partial step (if any): generic
        const bool more = kt + 1 < ns;
        if (more) gload(GEN, kt + 1);
        compute(kt & 1);
        if (more) split(GEN, kt + 1, (kt + 1) & 1);
        __syncthreads();
    }

    // ---- fp16x2 dynamic-range guard (as gi_gemm_bf3_kernel): rows of A whose largest SCALED magnitude is below 2^-11,
    // counted once per launch by the workgroups of the first column tile; zero rows are exact and not counted
    if (p.x2_guard && bx == 0) {
        int n_low = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float m = rowmax[i];
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));                     // the four lanes (k chunks) of a row
            const bool real_row = m0 + (tid >> 2) + 64 * i < m_end;
            n_low += (c8 == 0 && real_row && m > 0.f && m * sa < 0x1p-11f) ? 1 : 0;
        }
        if (n_low) {
            atomicAdd(p.x2_guard, n_low);
            if (p.x2_guard_host) *reinterpret_cast<volatile int*>(p.x2_guard_host) = 1;
        }
    }

    // ---- epilogue (C/D layout of a 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) --
    const int flags = EPI == 1 ? (GI_EPI_BIAS | GI_EPI_SELU) : GI_EPI_DSELU;
    const int col = n0 + 32 * wid + l31;
    const bool col_ok = col < p.N;
    const int colc = col_ok ? col : p.N - 1;
    const float bv = (flags & GI_EPI_BIAS) ? p.bias[colc] : 0.f;
    float amax[2] = {0.f, 0.f};                                  // rows 0-63 / 64-127 of the tile
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row0 = m0 + t * 32 + 4 * lhi;
        float av[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {                            // every load of the block before the first store
            const int row = min(row0 + 8 * (r >> 2) + (r & 3), m_end - 1);
            if (flags & GI_EPI_DSELU) av[r] = p.act[(long long)row * p.ldact + colc];
        }
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = (acc[t][r] * ia) * ib + bv;
            if (flags & GI_EPI_SELU) x = gi_selu(x);
            if (flags & GI_EPI_DSELU) x *= gi_selu_grad(av[r]);
            v[r] = x;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + 8 * (r >> 2) + (r & 3);
            const bool ok = col_ok & (row < m_end);
            float* dst = ok ? p.C + (long long)row * p.ldc + col : gi_sink + tid;
            *dst = v[r];
            amax[t >> 1] = fmaxf(amax[t >> 1], ok ? fabsf(v[r]) : 0.f);
        }
    }
    if (p.c_amax) {                   // the slots of gi_gemm_bf3_kernel's wave (wm, wn) = (half, wid >> 1) of this tile
        const int tiles = b.start[pi + 1] - b.start[pi];
        const int local = by * b.gx[pi] + bx;       // the workgroup gi_gemm_bf3_kernel would have run this tile with
        const int blk = b.start[pi] + (b.old_remap ? gi_xcd_remap_inv(local, tiles) : local);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            gx_amax_publish_slot(amax[h], p.c_amax, (blk * 4 + 2 * h + (wid >> 1)) & (GX_AMAX_SLOTS - 1));
    }
}

// gi_gemm_bf3_kernel's fp16x2 launches: both operands plain fp32 with k contiguous, both amax cells
constexpr GiGemmCaps XN_CAPS = {
    /*BM, BN*/ XN_BM, XN_BN, /*layouts*/ GI_LAY_CC, /*strip*/ GI_GEMM_BF3 | GI_GEMM_BF3A | GI_GEMM_BF3B_F32 | GI_GEMM_X2,
    /*epi_classes*/ 0x7, /*images*/ false, /*x2_layouts*/ GI_LAY_CC, /*x2_slabs_plain*/ false, /*a_idx*/ false,
    /*b_idx*/ GI_BIDX_NONE, /*k_dev*/ false, /*m_dev*/ true, /*ones_col*/ false, /*splitk_layouts*/ 0, /*groups*/ GI_GROUPS_NONE, /*need_ptrs*/ true,
    /*need_ld*/ true, /*even_major_ld*/ false, /*pad_major*/ false, /*limit_all*/ false, /*k_min*/ 1, /*order*/ GI_ORDER_NONE,
    /*limits_last*/ true, /*flags_last*/ false, /*bidx_last*/ false};

}  // namespace

// gi_gemm_bf3_launch hands fp16x2 launches of plain fp32 operands with the forward / dgrad epilogue here (validated
// there: every problem GI_GEMM_X2 | GI_GEMM_BF3B_F32, no gathers, both amax cells, 32-bit offsets)
int gi_x2n_launch(const gi_gemm_params* probs, int n, int epi, void* stream) {
    GiGemmBatch b;
    double flops;
    int e;
    if (int rc = gi_plan_build(probs, n, XN_CAPS, &b, &flops, &e)) return rc;
    if (e != epi || (epi != 1 && epi != 2)) return GI_EINVAL;
    if (b.n == 0) return 0;
    const int k = b.n, total = b.total;
    int grid = 0;
    for (int i = 0; i < k; ++i) grid += 8 * ((b.gy[i] + 7) / 8) * b.gx[i];   // room for every XCD's share, whatever the real row count
    b.old_remap = gi_order_rows(total, gi_plan_bounded(b)) ? 1 : 0;          // (for the c_amax slots)
    hipStream_t st = (hipStream_t)stream;
    GiProfScope prof(st, GI_PROF_GEMM | GI_PROF_PIPE_X2, flops);
    gi_gemm_log_launch(epi == 1 ? "x0" : "x1", b.p, k, total, flops);
    if (epi == 1) hipLaunchKernelGGL((gi_gemm_x2n_kernel<1>), dim3(grid), dim3(256), 0, st, b);
    else hipLaunchKernelGGL((gi_gemm_x2n_kernel<2>), dim3(grid), dim3(256), 0, st, b);
    return gi_launch_status();
}
