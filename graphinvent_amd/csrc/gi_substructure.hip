// Substructure search on the device (gfx950): which of G molecules contain which of P patterns, where, and how often —
// what a generator's user does today with one RDKit HasSubstructMatch per molecule and pattern on the host (structural
// alerts, functional-group counts, "is the scaffold still there").  THIS IS NOT SMARTS AND NOT RDKit'S MATCHER: a pattern
// is a connected labelled graph of at most 32 atoms with type / charge / degree / hydrogen predicates per atom and a set
// of bond types per bond; no ring or recursive predicates, no aromaticity perception (a Kekule pattern matches the
// molecule's stored Kekule phase only).  The semantics, the plan and the search order are written out in
// include/graphinvent_amd.h at gi_mol_substructure; tests/substructure_model.py is the specification, matched integer
// for integer.
//
// mol_substructure_kernel  one 256-lane WORKGROUP per molecule:
//   1, 2  gi_read_labelled<true> of gi_molread.h (the front end of gi_valence.hip, gi_fingerprint.hip, gi_smiles.hip):
//      every byte read once (fp32 or int8, any alignment), one 128-bit adjacency row per (bond type, node) in LDS, n given
//      or derived, the GI_MOL_MALFORMED / self-loop / empty bits (any of them: the molecule matches nothing);
//   3  one lane per atom: type index, charge index, number of bonded partners, hydrogen fill (0 for an atom over its
//      valence), packed into one word of LDS;
//   4  each WAVE owns the patterns wave, wave + 4, ...: it builds compat[k], the 128-bit mask of the atoms that satisfy
//      the predicates of plan position k, by ballots (every lane stores the same words and later reads what it stored
//      itself, so no ordering between lanes is needed), then each LANE searches from the anchors `lane` and `lane + 64`.
//      A lane's state: img[k] (one byte per position, LDS, [position][lane]), the 128-bit `used` mask, the position k, the
//      image just abandoned and the step count, in registers.  On backtracking the candidate mask is recomputed and cut
//      to "above the image just abandoned": there is no per-level stack.  A step is a handful of 128-bit ANDs and a ctz;
//      the plan row of a position is one 16-byte load from the pattern table in global memory (cache-resident).
//      The lanes of a wave diverge by construction; that is accepted.
//   5  match, n_anchors, anchors and n_limited come from ballots; `first` is written by the lane of the LOWEST matching
//      anchor (if one of the anchors 0..63 matches it is written before the second round overwrites img).
// Integers only, no global atomics, no scratch memory, nothing to clear in front of the launch.  Loops are bounded by N,
// Np, Fe, P and max_steps (a search takes at most 2 max_steps + 2 iterations: each takes a step or undoes one).  Every
// index is bounded by the dims: atoms < n <= N come out of masks cut to n, positions are clamped below k, table offsets
// are checked on the host (gi_sub_check_table) and clamped again where they index LDS.
// LDS, all of it dynamic so that every 128-bit row is 16-byte aligned: Fe N 16 B of adjacency rows (<= 16 KB) plus
// 15.9 KB: the OR rows (2 KB) and GiLabelled (3 KB) of the shared reader, compat (2 KB), img (8 KB), the atom words
// (0.5 KB).  That is twice the "adjacency rows plus about 8 KB" one would get without the shared reader's own state.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int MAXA = GI_SUB_MAX_ATOMS;
constexpr int WAVES = NT / 64;
constexpr int LABEL_BITS = GI_MOL_MALFORMED | GI_LABEL_EMPTY | GI_LABEL_SELF_LOOP;
constexpr int HDR = 8, REC = 4, ROW = 8;                     // words of the table's header, a record's and a row's head
constexpr size_t ST_BYTES = (sizeof(GiLabelled) + 15) & ~(size_t)15;
constexpr size_t FIXED_LDS = MAXN * 16 + WAVES * MAXA * 16 + WAVES * MAXA * 64 + MAXN * 4 + ST_BYTES + 16;

struct SubTable {
    const int* words;                                        // the packed patterns (gi_mol_substructure)
    int P, Npm, TW, CW, Bmax, R, S;
};

struct SubOut {
    int *match, *n_anchors, *anchors, *first, *n_limited, *status;
};

__host__ __device__ __forceinline__ u64 below64(int m) { return m <= 0 ? 0ull : m >= 64 ? ~0ull : (1ull << m) - 1ull; }
__host__ __device__ __forceinline__ int sub_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }
__host__ __device__ __forceinline__ bool sub_bit(const unsigned* row, int j) { return (row[j >> 5] >> (j & 31)) & 1u; }

// The search of one (molecule, pattern, anchor): 1 found, 2 none, 3 given up at max_steps.  rec / back: the pattern's
// record and back bonds; adj [Fe][N][4] and orr [N][4] the adjacency rows and their OR over the types; cw [Np] the
// compatible atoms per position; img[k * stride] the image of position k (this search's own bytes).
__host__ __device__ __forceinline__ int sub_search(const int* rec, const int* back, int R, int Bmax, int Np, unsigned fe_all,
                                                   int N, const unsigned* adj, const unsigned (*orr)[4], const uint4* cw,
                                                   unsigned char* img, int stride, int a0, int max_steps) {
    const uint4* adj4 = reinterpret_cast<const uint4*>(adj);
    const uint4* orr4 = reinterpret_cast<const uint4*>(orr);
    img[0] = (unsigned char)a0;
    if (Np == 1) return 1;
    u64 used_lo = a0 < 64 ? 1ull << a0 : 0ull, used_hi = a0 < 64 ? 0ull : 1ull << (a0 - 64);
    int k = 1, low = -1, steps = 0;
    const long long cap = 2ll * max_steps + 2;               // every iteration takes a step or undoes one
    for (long long it = 0; it < cap; ++it) {
        const int4 pl = *reinterpret_cast<const int4*>(rec + REC + k * R);            // parent, mask, back bonds
        const int pi = img[sub_clamp(pl.x, 0, k - 1) * stride];
        uint4 near = make_uint4(0u, 0u, 0u, 0u);
        unsigned pm = (unsigned)pl.y & fe_all;
        if (pm == fe_all) {
            near = orr4[pi];
        } else {
            while (pm) {
                const uint4 r = adj4[__builtin_ctz(pm) * N + pi];
                pm &= pm - 1;
                near.x |= r.x; near.y |= r.y; near.z |= r.z; near.w |= r.w;
            }
        }
        const uint4 cm = cw[k];
        const u64 cand_lo = (cm.x | ((u64)cm.y << 32)) & (near.x | ((u64)near.y << 32)) & ~used_lo & ~below64(low + 1);
        const u64 cand_hi = (cm.z | ((u64)cm.w << 32)) & (near.z | ((u64)near.w << 32)) & ~used_hi & ~below64(low - 63);
        if ((cand_lo | cand_hi) == 0ull) {                   // nothing left here: back to the position before
            if (--k == 0) return 2;
            low = img[k * stride];
            if (low < 64) used_lo &= ~(1ull << low); else used_hi &= ~(1ull << (low - 64));
            continue;
        }
        if (steps == max_steps) return 3;
        ++steps;
        const int c = cand_lo ? __builtin_ctzll(cand_lo) : 64 + __builtin_ctzll(cand_hi);
        bool ok = true;
        const int b0 = sub_clamp(pl.z, 0, Bmax), b1 = sub_clamp(pl.w, 0, Bmax - b0) + b0;
        for (int b = b0; b < b1 && ok; ++b) {                // the back bonds
            const int e = back[b];
            const int qi = img[sub_clamp(e & 31, 0, k - 1) * stride];
            unsigned bm = (unsigned)(e >> 8) & fe_all;
            bool hit = false;
            if (bm == fe_all) {
                hit = sub_bit(orr[c], qi);
            } else {
                while (bm) {
                    hit |= sub_bit(adj + (__builtin_ctz(bm) * N + c) * 4, qi);
                    bm &= bm - 1;
                }
            }
            ok = hit;
        }
        if (!ok) { low = c; continue; }
        img[k * stride] = (unsigned char)c;
        if (c < 64) used_lo |= 1ull << c; else used_hi |= 1ull << (c - 64);
        if (k == Np - 1) return 1;
        ++k;
        low = -1;
    }
    return 3;                                                // not reached
}

template <typename T>
__global__ __launch_bounds__(NT) void mol_substructure_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                              const void* __restrict__ n_nodes, int nn_bytes, int N,
                                                              int Fn, int Fe, int A, int C, int H,
                                                              const unsigned short* __restrict__ allowed,
                                                              const i8* __restrict__ order2, SubTable tb,
                                                              const int* __restrict__ pattern_index, int max_steps,
                                                              SubOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* adj = reinterpret_cast<unsigned*>(smem);                   // [Fe][N][4]
    unsigned(*orr)[4] = reinterpret_cast<unsigned(*)[4]>(adj + Fe * N * 4);
    uint4* compat = reinterpret_cast<uint4*>(orr + MAXN);                // [WAVES][MAXA]
    unsigned char* img = reinterpret_cast<unsigned char*>(compat + WAVES * MAXA);     // [WAVES][MAXA][64]
    int* prop = reinterpret_cast<int*>(img + WAVES * MAXA * 64);         // [MAXN]: type | charge << 10 | degree << 20 | h << 28
    GiLabelled& st = *reinterpret_cast<GiLabelled*>(prop + MAXN);
    int* limited_sh = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(&st) + ST_BYTES);

    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    if (tid == 0) *limited_sh = 0;

    // ---- 1, 2: read and check ---------------------------------------------------------------------------------
    GiLabelledNode me;
    const int n = gi_read_labelled<true>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes, nn_bytes,
                                         g, N, Fn, Fe, A, C, H, order2, tid, adj, st, orr, me);
    const int label = st.flags & LABEL_BITS;                 // uniform
    const bool sound = label == 0;

    // ---- 3: the atoms' words ------------------------------------------------------------------------------------
    if (sound && tid < n) {
        const int a = st.seg_first[0][tid], c = st.seg_first[1][tid];     // a < A, c < C: the row is one-hot
        const int h = max(gi_hydrogen_fill((unsigned)allowed[a * C + c], (me.o2 + 1) >> 1), 0);      // <= 15
        prop[tid] = a | (c << 10) | (min(me.deg, 255) << 20) | (h << 28);
    }
    __syncthreads();

    // ---- 4, 5: the wave's patterns ------------------------------------------------------------------------------
    const int Pout = pattern_index ? 1 : tb.P;
    const int pidx = pattern_index ? pattern_index[g] : 0;
    const bool bad_index = pattern_index && (pidx < 0 || pidx >= tb.P);
    const unsigned fe_all = (1u << Fe) - 1u;                 // Fe <= 8
    unsigned char* my = img + wave * (MAXA * 64) + lane;     // my[k * 64]: the image of position k
    uint4* cw = compat + wave * MAXA;
    for (int col = wave; col < Pout; col += WAVES) {
        const int p = pattern_index ? pidx : col;
        const size_t o = (size_t)g * Pout + col;
        int* first = out.first + o * tb.Npm;
        if (!sound || bad_index) {                           // uniform
            if (lane == 0) {
                out.match[o] = out.n_anchors[o] = out.n_limited[o] = 0;
                for (int w = 0; w < 4; ++w) out.anchors[o * 4 + w] = 0;
            }
            if (lane < tb.Npm) first[lane] = -1;
            continue;
        }
        const int* rec = tb.words + HDR + (size_t)p * tb.S;
        const int* back = rec + REC + tb.Npm * tb.R;
        const int Np = min(max(rec[0], 1), tb.Npm);
        for (int k = 0; k < Np; ++k) {                       // compat[k]
            const int* row = rec + REC + k * tb.R;
            const int deg = row[5], mh = row[6];
            unsigned m[4] = {0u, 0u, 0u, 0u};
            for (int half = 0; half < 2 && 64 * half < n; ++half) {
                const int i = lane + 64 * half;
                bool ok = false;
                if (i < n) {
                    const int pr = prop[i], a = pr & 1023, c = (pr >> 10) & 1023, d = (pr >> 20) & 255, h = (pr >> 28) & 15;
                    ok = ((row[ROW + (a >> 5)] >> (a & 31)) & 1) && ((row[ROW + tb.TW + (c >> 5)] >> (c & 31)) & 1) &&
                         (deg < 0 || d == deg) && (mh < 0 || h >= mh);
                }
                const u64 b = __ballot(ok);
                m[2 * half] = (unsigned)b;
                m[2 * half + 1] = (unsigned)(b >> 32);
            }
            cw[k] = make_uint4(m[0], m[1], m[2], m[3]);      // the same words from every lane
        }
        unsigned anc[4] = {0u, 0u, 0u, 0u};
        int n_limited = 0;
        bool have_first = false;
        for (int half = 0; half < 2 && 64 * half < n; ++half) {
            const int a0 = lane + 64 * half;
            int res = 0;                                     // 1: found, 2: none, 3: given up
            const uint4 c0 = cw[0];
            const u64 c0lo = c0.x | ((u64)c0.y << 32), c0hi = c0.z | ((u64)c0.w << 32);
            if (a0 < n && (((half ? c0hi : c0lo) >> lane) & 1ull))
                res = sub_search(rec, back, tb.R, tb.Bmax, Np, fe_all, N, adj, orr, cw, my, 64, a0, max_steps);
            const u64 f = __ballot(res == 1), l = __ballot(res == 3);
            anc[2 * half] = (unsigned)f;
            anc[2 * half + 1] = (unsigned)(f >> 32);
            n_limited += __popcll(l);
            if (f && !have_first) {                          // uniform: the lowest matching anchor's lane
                have_first = true;
                if (lane == __builtin_ctzll(f)) {
                    for (int k = Np; k < tb.Npm; ++k) first[k] = -1;
                    for (int k = 0; k < Np; ++k) first[min(rec[REC + k * tb.R + 4] & 31, Np - 1)] = my[k * 64];
                }
            }
        }
        if (!have_first && lane < tb.Npm) first[lane] = -1;
        if (lane == 0) {
            const int cnt = __popc(anc[0]) + __popc(anc[1]) + __popc(anc[2]) + __popc(anc[3]);
            out.match[o] = cnt > 0;
            out.n_anchors[o] = cnt;
            out.n_limited[o] = n_limited;
            for (int w = 0; w < 4; ++w) out.anchors[o * 4 + w] = (int)anc[w];
            if (n_limited) atomicOr(limited_sh, 1);          // LDS
        }
    }
    __syncthreads();
    if (tid == 0)
        out.status[g] = label | (*limited_sh ? GI_SUB_STEP_LIMIT : 0) | (bad_index ? GI_SUB_PATTERN_INDEX : 0);
}

// bits [0, k) of the words w[0, ceil(k / 32)) only
bool bits_within(const int* w, int words, int k) {
    for (int i = 0; i < words; ++i) {
        const int r = k - 32 * i;
        const unsigned ok = r >= 32 ? ~0u : r <= 0 ? 0u : (1u << r) - 1u;
        if ((unsigned)w[i] & ~ok) return false;
    }
    return true;
}

}  // namespace

// The host copy of a pattern table against its own header and the caller's dims: 0, GI_EINVAL or GI_ELIMIT.
static int gi_sub_check_table(const int* t, long long words, int n_types, int n_charges, int Fe, SubTable* tb) {
    if (words < HDR) return GI_EINVAL;
    const int P = t[0], Npm = t[1], TW = t[5], CW = t[6], Bmax = t[7];
    if (P < 1 || Npm < 1 || t[2] != n_types || t[3] != n_charges || t[4] != Fe) return GI_EINVAL;
    if (Npm > GI_SUB_MAX_ATOMS || P > GI_SUB_MAX_PATTERNS) return GI_ELIMIT;
    if (TW != (n_types + 31) / 32 || CW != (n_charges + 31) / 32 || Bmax < 0 || Bmax > gi_r4(Npm * (Npm - 1) / 2) ||
        (Bmax & 3))
        return GI_EINVAL;
    const int R = ROW + gi_r4(TW + CW), S = REC + Npm * R + Bmax;
    if (words != HDR + (long long)P * S) return GI_EINVAL;
    const unsigned fe_all = (1u << Fe) - 1u;
    for (int p = 0; p < P; ++p) {
        const int* rec = t + HDR + (long long)p * S;
        const int* back = rec + REC + Npm * R;
        const int Np = rec[0];
        if (Np < 1 || Np > Npm) return GI_EINVAL;
        unsigned seen = 0u;
        for (int k = 0; k < Np; ++k) {
            const int* row = rec + REC + k * R;
            const int parent = row[0], pmask = row[1], b0 = row[2], bc = row[3], atom = row[4];
            if (atom < 0 || atom >= Np || ((seen >> atom) & 1u)) return GI_EINVAL;       // the plan is a permutation
            seen |= 1u << atom;
            if (k == 0 ? (parent != 0 || pmask != 0 || bc != 0) : (parent < 0 || parent >= k)) return GI_EINVAL;
            if (k > 0 && (pmask == 0 || ((unsigned)pmask & ~fe_all))) return GI_EINVAL;
            if (b0 < 0 || bc < 0 || b0 > Bmax || bc > Bmax - b0) return GI_EINVAL;
            for (int b = b0; b < b0 + bc; ++b) {
                const int q = back[b] & 0xff, m = back[b] >> 8;
                if (q >= k || q == parent || m == 0 || ((unsigned)m & ~fe_all)) return GI_EINVAL;
            }
            if (row[5] < -1 || row[5] > GI_MAX_NODES - 1 || row[6] < -1 || row[6] > 15) return GI_EINVAL;
            if (!bits_within(row + ROW, TW, n_types) || !bits_within(row + ROW + TW, CW, n_charges)) return GI_EINVAL;
        }
    }
    *tb = {nullptr, P, Npm, TW, CW, Bmax, R, S};
    return 0;
}

extern "C" int gi_mol_substructure(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                                   const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                                   const unsigned short* allowed, const signed char* order2, const int* patterns_host,
                                   const int* patterns, long long pattern_words, const int* pattern_index,
                                   int max_steps, int* match, int* n_anchors, int* anchors, int* first, int* n_limited,
                                   int* status, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if (max_steps < 1) return GI_EINVAL;
    if (max_steps > GI_SUB_MAX_STEPS) return GI_ELIMIT;
    SubTable tb = {};
    if (patterns_host)
        if (const int rc = gi_sub_check_table(patterns_host, pattern_words, n_types, n_charges, Fe, &tb)) return rc;
    if (G == 0) return 0;
    if (!nodes || !edges || !allowed || !order2 || !patterns_host || !patterns || ((uintptr_t)patterns & 15) || !match ||
        !n_anchors || !anchors || !first || !n_limited || !status)
        return GI_EINVAL;
    tb.words = patterns;
    const SubOut out = {match, n_anchors, anchors, first, n_limited, status};
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned) + FIXED_LDS;                          // <= 32 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_substructure_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, allowed,
                           order2, tb, pattern_index, max_steps, out);
    else
        hipLaunchKernelGGL(mol_substructure_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, allowed, order2, tb,
                           pattern_index, max_steps, out);
    return gi_launch_status();
}
