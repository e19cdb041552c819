// Launch plan and tile decode of the GEMM kernel family (gi_gemm.hip, gi_gemm_bf3.hip, gi_gemm_x2n.hip,
// gi_gemm_b3v.hip, gi_gemm_b3p.hip): what a launcher accepts (one GiGemmCaps row per file), the descriptor checks, the
// tile grid, the tile-order rules and — for the kernels — tile id -> tile.  The k loops stay in their files.
//
// HOST PART: plain C++17 on graphinvent_amd.h and the C library (no HIP header, no HIP call: tests compile it alone).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "graphinvent_amd.h"

#define GI_GEMM_BATCH_MAX 8
// Several independent problems of one tile / layout class in ONE launch; tile id -> (problem, x, y, z) through the
// prefix table `start`.  (Kernel argument of every kernel of the family; a kernel ignores the fields it has no use for.)
struct GiGemmBatch {
    gi_gemm_params p[GI_GEMM_BATCH_MAX];
    int start[GI_GEMM_BATCH_MAX + 1];          // first tile id of every problem
    int gx[GI_GEMM_BATCH_MAX], gy[GI_GEMM_BATCH_MAX];
    int n, total;
    int remap;                                 // XCD-aware tile order over each problem's tile list (gi_xcd_remap)
    int old_remap;                             // gi_gemm_x2n.hip: the order gi_gemm_bf3_kernel would have used (c_amax slots)
};

// gi_gemm.hip keeps its two tile orders in p.flags of the batch (per problem).  The values overlap PUBLIC routing bits
// (2048 is GI_GEMM_T128): safe only because gi_plan_check rejects, on entry, every public bit the fp32 row does not
// strip or know — no descriptor reaches the kernel with one of them set by the caller.
enum { GI_TILES_ROW_ORDER = 32, GI_TILES_SLAB_ORDER = 2048 };
enum { GI_EPI_ALL = GI_EPI_BIAS | GI_EPI_SELU | GI_EPI_DSELU | GI_EPI_ACCUM | GI_EPI_MULACT };
static_assert(((GI_TILES_ROW_ORDER | GI_TILES_SLAB_ORDER) & (GI_EPI_ALL | GI_GEMM_SPLITK)) == 0,
              "the internal tile-order bits must not collide with a flag the fp32 kernel reads");
static_assert(GI_TILES_SLAB_ORDER == GI_GEMM_T128, "documented overlap: see the comment above before changing either");

enum { GI_LAY_CC = 1, GI_LAY_CM = 2, GI_LAY_MM = 4 };      // A / B contig or major ([reduction][rows])
static inline int gi_layout_of(const gi_gemm_params& p) {
    return p.a_major ? (p.b_major ? GI_LAY_MM : 0) : (p.b_major ? GI_LAY_CM : GI_LAY_CC);
}
enum { GI_BIDX_NONE, GI_BIDX_MAJOR, GI_BIDX_X2_SLABS };
enum { GI_GROUPS_NONE, GI_GROUPS_SLABS, GI_GROUPS_ANY };
// tile order: none / gi_gemm.hip's two (in p.flags) / gi_order_rows on non-a_major launches / ... and gi_order_slabs on
// a_major ones / ... on the fp16x2 ones among them only
enum { GI_ORDER_NONE, GI_ORDER_TILES, GI_ORDER_ROWS, GI_ORDER_ROWS_SLABS, GI_ORDER_ROWS_X2SLABS };

// What one launcher accepts.  The last three fields only keep which of two errors a doubly malformed descriptor
// gets, as each launcher has answered so far.
struct GiGemmCaps {
    int BM, BN;                  // block tile; 0 = 64 tm x 64 tn of the descriptor (tm, tn checked)
    int layouts;                 // GI_LAY_*
    int strip;                   // routing bits taken out of flags; any other bit beyond GI_EPI_* / SPLITK: GI_EINVAL
    int epi_classes;             // bit e: epilogue class e has its own instantiation (class 0 = run-time flags);
                                 // 0: "own" mode — 1 when every problem has its layout's own epilogue, else 0
    bool images;                 // pre-split operand images (GI_GEMM_BF3A; a contig B without GI_GEMM_BF3B_F32),
                                 // 16-byte aligned; without: operands are fp32 matrices
    int x2_layouts;              // GI_GEMM_X2 on these layouts (needs both amax cells, every problem or none)
    bool x2_slabs_plain;         // fp16x2 split-K: flag-free epilogue only
    bool a_idx;
    int b_idx;                   // GI_BIDX_*: never / on a major B / fp16x2 weight-gradient slabs, every problem or none
    bool k_dev, m_dev;           // (m_dev never with split-K or groups)
    bool ones_col;               // a major B may end in the ones column (without: the field is not read at all)
    int splitk_layouts;          // GI_GEMM_SPLITK on these layouts
    int groups;                  // GI_GROUPS_*
    bool need_ptrs;              // A, B and (ungrouped) C non-null
    bool need_ld;                // contig: ld >= K; major: ld >= stored columns >= 1
    bool even_major_ld;          // major operands are read as 8-byte column pairs: ld >= columns rounded up to even
    bool pad_major;              // major operands narrower than 4 columns need ld >= 4
    bool limit_all;              // 32-bit offsets on major operands, C and act too (else contig operands only)
    int k_min;
    int order;                   // GI_ORDER_*: which tile-order rule gi_plan_build applies
    bool limits_last;            // B's GI_EINVAL checks before A's GI_ELIMIT
    bool flags_last;             // unknown flag bits are checked after the limits
    bool bidx_last;              // the b_idx rules are checked after every problem's other checks and the tile limit
};

// ---- tile-order rules, each stated once ------------------------------------------------------------------------------
// bf3 family (gi_gemm_bf3.hip; b3v / b3p for their non-a_major launches; x2n for old_remap): measured on the node-level
// hidden-layer launch (684 tiles): 76.7 -> 73.0 us forward, 84.0 -> 82.1 dgrad.  (bounded: the order would be over
// the bound's tiles)
static inline bool gi_order_rows(int total, bool bounded) { return total >= 512 && !bounded; }
// Weight-gradient launches (split-K slabs): consecutive tile ids are the column / row tiles of ONE slab, i.e. the
// workgroups that read the SAME rows of both operands — dealt round-robin to the 8 XCDs each of them pulls its columns
// of those rows through a different L2 (2.5-3.1 x the operand bytes per launch through the fabric).  With the bijective
// remap one XCD walks consecutive ids: a slab's tiles share an L2.
static inline bool gi_order_slabs(bool a_major, int total, bool bounded) { return a_major && !bounded && total >= 16; }
// gi_gemm.hip: XCD-aware order inside a slab / a problem for launches of more than ~1.3 full rounds of 256 CUs x 4
// resident workgroups.  Measured on the training step (3 A/B pairs): never 2.74 ms, always 2.76-2.77 ms, >= 1300..2100
// workgroups 2.70-2.71 ms.  The small launches lose with the remap (an XCD's share of a 1-round launch is not
// balanced), the big ones win (column tiles sharing an A row panel hit one L2).
static inline bool gi_order_tiles_rows(long long blocks) { return blocks >= 1350; }
// ... and the slab-per-XCD order over a split-K problem's whole tile list
static inline bool gi_order_tiles_slabs(int total, const gi_gemm_params& p) {
    return total >= 64 && (p.flags & GI_GEMM_SPLITK) && !p.m_dev;
}

// Epilogue class of the flags left after the routing bits: 1 = bias + SELU (forward), 2 = * selu'(act) (dgrad),
// 3 = plain store (weight-gradient slabs), 0 = anything else (run-time flags)
static inline int gi_epi_class(int f, bool splitk) {
    if (splitk) return f == 0 ? 3 : 0;
    return f == (GI_EPI_BIAS | GI_EPI_SELU) ? 1 : (f == GI_EPI_DSELU ? 2 : (f == 0 ? 3 : 0));
}

static inline int gi_plan_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int gi_plan_r32(int k) { return (k + 31) & ~31; }

static inline int gi_plan_bidx_check(const gi_gemm_params& p, const gi_gemm_params& p0, const GiGemmCaps& c) {
    if (!p.b_idx && c.b_idx != GI_BIDX_X2_SLABS) return 0;
    if (c.b_idx == GI_BIDX_NONE) return GI_EINVAL;
    if (c.b_idx == GI_BIDX_MAJOR) return p.b_major ? 0 : GI_EINVAL;
    if ((p.b_idx != nullptr) != (p0.b_idx != nullptr)) return GI_EINVAL;
    if (p.b_idx && !(p.a_major && p.b_major && (p.flags & GI_GEMM_X2) && (p.flags & GI_GEMM_SPLITK))) return GI_EINVAL;
    return 0;
}

// The descriptor checks of one problem (p0: the launch's first problem, for the every-problem-or-none rules)
static inline int gi_plan_check(const gi_gemm_params& p, const gi_gemm_params& p0, const GiGemmCaps& c) {
    const bool splitk = (p.flags & GI_GEMM_SPLITK) != 0;
    const bool x2 = (p.flags & c.strip & GI_GEMM_X2) != 0;
    const bool a_img = c.images && (p.flags & GI_GEMM_BF3A), b_img = c.images && !(p.flags & GI_GEMM_BF3B_F32);
    const int lay = gi_layout_of(p);
    if (c.need_ptrs && (!p.A || !p.B)) return GI_EINVAL;
    if (p.M < 0 || p.N <= 0 || p.K < c.k_min || p.nsplit < 1 || p.ngroups < 0 || p.ngroups > GI_MAX_GROUPS)
        return GI_EINVAL;
    if (!(lay & c.layouts)) return GI_EINVAL;
    if (!c.BM && !((p.tm == 1 && p.tn == 1) || (p.tm == 1 && p.tn == 2) || (p.tm == 2 && p.tn == 2))) return GI_EINVAL;
    if (!splitk && p.nsplit != 1) return GI_EINVAL;
    if (p.ngroups && (!p.grp_off || c.groups == GI_GROUPS_NONE || (c.groups == GI_GROUPS_SLABS && !splitk))) return GI_EINVAL;
    if (c.need_ptrs && !p.ngroups && !p.C) return GI_EINVAL;
    if (splitk && (!(lay & c.splitk_layouts) || p.m_dev || p.k_dev)) return GI_EINVAL;
    if ((p.m_dev && (!c.m_dev || p.ngroups)) || (p.k_dev && (!c.k_dev || p.ngroups))) return GI_EINVAL;
    if (p.a_idx && (!c.a_idx || p.a_major)) return GI_EINVAL;
    if (c.ones_col && p.ones_col >= 0 && (!p.b_major || p.ones_col != p.N - 1)) return GI_EINVAL;
    if (splitk && p.ngroups)
        for (int g = 0; g < p.ngroups; ++g)
            if (p.gsplit[g] < 1) return GI_EINVAL;
    const int f = p.flags & ~(c.strip | GI_GEMM_SPLITK);
    const bool bad_flags = (f & ~GI_EPI_ALL) != 0;
    if (bad_flags && !c.flags_last) return GI_EINVAL;
    if (c.need_ptrs && (((f & GI_EPI_BIAS) && !p.bias) || ((f & (GI_EPI_DSELU | GI_EPI_MULACT)) && !p.act))) return GI_EINVAL;
    if (((p.flags ^ p0.flags) & c.strip & GI_GEMM_X2) != 0) return GI_EINVAL;
    if (c.images && (((p.flags ^ p0.flags) & (GI_GEMM_BF3A | GI_GEMM_BF3B_F32)) != 0)) return GI_EINVAL;
    if (x2 && (!(lay & c.x2_layouts) || a_img || b_img || !p.a_amax || !p.b_amax || (c.x2_slabs_plain && splitk && f != 0)))
        return GI_EINVAL;
    if (!c.bidx_last)
        if (int rc = gi_plan_bidx_check(p, p0, c)) return rc;
    // Operands.  An image: 16-byte aligned.  A contig fp32 operand: rows narrower than one 16-byte vector are stored
    // padded to 4 floats.  A major one: its stored columns (B: without the ones column) fit its leading dimension.
    auto contig_bad = [&](int ld) { return (c.need_ld && ld < p.K) || (p.K < 4 && ld < 4); };
    auto major_bad = [&](int cols, int pad_cols, int ld) {
        return (c.need_ld && (ld < cols + (c.even_major_ld ? (cols & 1) : 0) || cols < 1)) || (c.pad_major && pad_cols < 4 && ld < 4);
    };
    const int bcols = (c.ones_col && p.ones_col >= 0) ? p.ones_col : p.N;
    const bool a_bad = a_img ? ((uintptr_t)p.A & 15) != 0 : (p.a_major ? major_bad(p.M, p.M, p.lda) : contig_bad(p.lda));
    const bool b_bad = b_img ? ((uintptr_t)p.B & 15) != 0 : (p.b_major ? major_bad(bcols, p.N, p.ldb) : contig_bad(p.ldb));
    // 32-bit byte offsets inside every matrix the kernels address that way
    const long long lim = 0xffffffffLL / 4;
    const bool a_lim = (!p.a_major || c.limit_all) && !p.a_idx && (long long)(p.a_major ? p.K : p.M) * p.lda > lim;
    bool b_lim = !b_img && (!p.b_major || c.limit_all) && !p.b_idx && (long long)(p.b_major ? p.K : p.N) * p.ldb > lim;
    if (c.images && (long long)p.N * gi_plan_r32(p.K) * 2 > 0xffffffffLL) b_lim = true;       // (the extent of B's image)
    if (c.limit_all && ((long long)p.M * p.ldc > lim || (p.act && (long long)p.M * p.ldact > lim))) b_lim = true;
    if (a_bad) return GI_EINVAL;
    if (c.limits_last) { if (b_bad) return GI_EINVAL; if (a_lim || b_lim) return GI_ELIMIT; }
    else { if (a_lim) return GI_ELIMIT; if (b_bad) return GI_EINVAL; if (b_lim) return GI_ELIMIT; }
    if (bad_flags) return GI_EINVAL;
    // every problem of a launch: the same layout and tile shape
    if (lay != gi_layout_of(p0) || (!c.BM && (p.tm != p0.tm || p.tn != p0.tn))) return GI_EINVAL;
    return 0;
}

static inline bool gi_plan_bounded(const GiGemmBatch& b) {
    bool bounded = false;
    for (int i = 0; i < b.n; ++i) bounded |= b.p[i].m_dev != nullptr;
    return bounded;
}

// Fills the batch from the problems a launcher was handed (in `order`, if given): checks, M == 0 problems skipped, tile
// grid, routing bits stripped, tile order.  *epi: the epilogue class every problem shares (0: run-time flags).
// Returns 0 (b->n == 0: nothing to launch), GI_EINVAL or GI_ELIMIT.
static inline int gi_plan_build(const gi_gemm_params* probs, int n, const GiGemmCaps& c, GiGemmBatch* b, double* flops,
                                int* epi, const int* order = nullptr) {
    memset(b, 0, sizeof(*b));
    *flops = 0;
    *epi = -1;
    if (!probs || n < 1 || n > GI_GEMM_BATCH_MAX) return GI_EINVAL;
    int total = 0, k = 0;
    for (int ii = 0; ii < n; ++ii) {
        const gi_gemm_params& p = probs[order ? order[ii] : ii];
        if (int rc = gi_plan_check(p, probs[0], c)) return rc;
        const bool splitk = (p.flags & GI_GEMM_SPLITK) != 0;
        const int f = p.flags & ~(c.strip | GI_GEMM_SPLITK);
        int e;
        if (c.epi_classes) { e = gi_epi_class(f, splitk); if (!((c.epi_classes >> e) & 1)) e = 0; }
        else e = gi_epi_class(f, false) == (p.a_major ? 3 : (p.b_major ? 2 : 1));
        *epi = (*epi < 0 || *epi == e) ? e : 0;
        const int rows = splitk ? p.M : (p.ngroups ? p.max_group_rows : p.M);
        if (rows <= 0) continue;
        int zs = p.ngroups ? p.ngroups : 1;
        if (splitk) {
            zs = p.nsplit;
            if (p.ngroups) { zs = 0; for (int g = 0; g < p.ngroups; ++g) zs += p.gsplit[g]; }
        }
        b->p[k] = p; b->p[k].flags = f | (splitk ? GI_GEMM_SPLITK : 0);
        b->gx[k] = gi_plan_cdiv(p.N, c.BN ? c.BN : 64 * p.tn); b->gy[k] = gi_plan_cdiv(rows, c.BM ? c.BM : 64 * p.tm);
        b->start[k] = total;
        if ((long long)b->gx[k] * b->gy[k] * zs + total > 0x3fffffff) return GI_ELIMIT;
        total += b->gx[k] * b->gy[k] * zs;
        *flops += 2.0 * (double)p.M * (double)p.N * (double)p.K;
        ++k;
    }
    if (c.bidx_last)
        for (int i = 0; i < n; ++i)
            if (int rc = gi_plan_bidx_check(probs[i], probs[0], c)) return rc;
    if (k == 0) { b->n = 0; return 0; }
    b->start[k] = total; b->n = k; b->total = total;
    const bool bounded = gi_plan_bounded(*b), am = b->p[0].a_major != 0, x2 = (probs[0].flags & c.strip & GI_GEMM_X2) != 0;
    if (c.order == GI_ORDER_TILES) {
        for (int i = 0; i < k; ++i) {
            if (gi_order_tiles_rows(total)) b->p[i].flags |= GI_TILES_ROW_ORDER;
            if (gi_order_tiles_slabs(total, b->p[i])) b->p[i].flags |= GI_TILES_SLAB_ORDER;
        }
    } else if (c.order != GI_ORDER_NONE) {
        b->remap = gi_order_rows(total, bounded) && !am;
        if ((c.order == GI_ORDER_ROWS_SLABS || (c.order == GI_ORDER_ROWS_X2SLABS && x2)) && gi_order_slabs(am, total, bounded))
            b->remap = 1;
    }
    return 0;
}

// Can a launcher of the 32-deep-tile kernels (b3v, b3p rows) take this GI_GEMM_BF3 launch from gi_gemm_bf3_launch?
// The routing questions of gi_plan_check: operand forms, layouts, gathers — not the malformed-descriptor ones.
static inline bool gi_plan_routable(const gi_gemm_params* probs, int n, const GiGemmCaps& c) {
    for (int i = 0; i < n; ++i) {
        const gi_gemm_params& p = probs[i];
        const int lay = gi_layout_of(p);
        if (!(p.flags & GI_GEMM_BF3) || (p.flags & GI_GEMM_BF3A)) return false;
        if (!(lay & c.layouts) || lay != gi_layout_of(probs[0])) return false;
        if (((p.flags ^ probs[0].flags) & GI_GEMM_X2) != 0) return false;
        if ((p.flags & GI_GEMM_X2) && (!(lay & c.x2_layouts) || !p.a_amax || !p.b_amax)) return false;
        if (!p.b_major && !(p.flags & GI_GEMM_BF3B_F32)) return false;      // contig B must be plain fp32, not an image
        if ((p.a_idx && !c.a_idx) || (p.k_dev && !c.k_dev)) return false;
        if (gi_plan_bidx_check(p, probs[0], c)) return false;
    }
    return true;
}

// The process-wide measurement switches (gi_b3v_enable, gi_b3p_enable, gi_x2_enable, gi_bf3_enable): the first use
// reads the environment (unset: dflt), on >= 0 sets, on < 0 only queries; returns the previous value.
static inline int gi_env_switch(int& state, const char* env, int dflt, int on) {
    if (state < 0) {
        const char* e = getenv(env);
        state = e ? (atoi(e) != 0) : dflt;
    }
    const int prev = state;
    if (on >= 0) state = on ? 1 : 0;
    return prev;
}

// ---- DEVICE PART --------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
// Where out-of-range lanes of edge tiles store (indexed by thread id; one instance per translation unit).
// GI_SINK_EXTERNAL (defined by gi_gemm.hip before this header): the instance gets external linkage.  With internal
// linkage the compiler sees that nothing ever reads the array, deletes the stores to it and turns `*(ok ? dst : sink) = v`
// into a store under a branch — a basic-block boundary per output element, at which it drains vmcnt(0).  The fp32
// kernel's epilogue is written around the unconditional store; the bf16x3 / fp16x2 kernels were tuned as they are.
#ifdef GI_SINK_EXTERNAL
__device__ float gi_sink[512];
#else
namespace {
__device__ float gi_sink[512];
}
#endif

// XCD-aware tile order, bijective on [0, tiles): consecutive workgroup ids go round-robin to the 8 XCDs (private L2
// each); the remap lets one XCD walk consecutive tiles, so the column tiles that share an A row panel hit one L2.
__device__ __forceinline__ int gi_xcd_remap(int local, int tiles) {
    const int q = tiles >> 3, r = tiles & 7, xcd = local & 7, j = local >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
// ... and the workgroup id that gi_xcd_remap sends to tile `local`
__device__ __forceinline__ int gi_xcd_remap_inv(int local, int tiles) {
    const int q = tiles >> 3, r = tiles & 7;
    int xcd, j;
    if (local < r * (q + 1)) { xcd = local / (q + 1); j = local - xcd * (q + 1); }
    else { const int l = local - r * (q + 1); xcd = r + l / q; j = l - (xcd - r) * q; }
    return j * 8 + xcd;
}

// Block-uniform description of an output tile.  m0 >= m_end: a tile beyond the rows on the device (bounded launch).
struct GiTile {
    int pi, bx, by, m0, n0, m_end, kb, ke;
    float* Cp;
};
// SLABS: the kernel runs split-K launches (plain or grouped slabs, reduction chunks rounded up to 32)
template <int BM, int BN, bool SLABS>
__device__ __forceinline__ GiTile gi_tile_decode(const GiGemmBatch& b, const int tile_id) {
    GiTile t;
    int pi = 0;
    while (pi < b.n - 1 && tile_id >= b.start[pi + 1]) ++pi;
    const gi_gemm_params& p = b.p[pi];
    int local = tile_id - b.start[pi];
    if (b.remap) local = gi_xcd_remap(local, b.start[pi + 1] - b.start[pi]);
    const int gx = b.gx[pi];
    int bz = 0, rem = local;
    if (SLABS) {
        const int gxy = gx * b.gy[pi];
        bz = local / gxy;
        rem = local - bz * gxy;
    }
    t.pi = pi;
    t.by = rem / gx; t.bx = rem - t.by * gx;
    t.m_end = p.m_dev ? min(p.M, *p.m_dev) : p.M;
    t.m0 = t.by * BM; t.n0 = t.bx * BN;
    t.kb = 0; t.ke = p.K;
    t.Cp = p.C;
    if (SLABS && (p.flags & GI_GEMM_SPLITK)) {      // reduction range of this slab
        int g = 0, s = bz, nsp = p.nsplit;
        if (p.ngroups) {
            while (g < p.ngroups - 1 && s >= p.gsplit[g]) { s -= p.gsplit[g]; ++g; }
            nsp = p.gsplit[g];
            t.Cp = p.Cg[g];
            t.kb = p.grp_off[g]; t.ke = p.grp_off[g + 1];
        }
        const int chunk = (((t.ke - t.kb + nsp - 1) / nsp) + 31) & ~31;
        t.kb += s * chunk;
        t.ke = min(t.kb + chunk, t.ke);
        t.Cp += (long long)s * p.c_split_stride;
    }
    return t;
}
#endif
