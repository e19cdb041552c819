// Molecule scores on the device (gfx950): a packed circular fingerprint per molecule, and a batch of fingerprints against
// a stored set (nearest neighbour by Tanimoto, kernel sums of a QSAR model) — what the reference's "activity" score
// (ScoringFunction.py:145-192) does per molecule on the host through RDKit and scikit-learn.  THE FINGERPRINT IS A
// MORGAN-STYLE FINGERPRINT OF THE LABELLED GRAPH, NOT RDKit's ECFP BITS: other atom invariants (no ring membership, no
// isotope, hydrogens only through the bond-order sum), another hash, no removal of duplicate substructures, no
// aromaticity perception.  A model must be trained on THESE fingerprints.  tests/fingerprint_model.py is the numpy
// specification; K0 / K1 are copied from it.
//
// mol_fingerprint_kernel  one 256-lane WORKGROUP per molecule:
//   1  read and check: gi_read_labelled of gi_molread.h, the front end shared with gi_valence.hip and gi_smiles.hip
//      (one 128-bit adjacency row per (bond type, node) in LDS, the bits of GI_MOL_MALFORMED, GI_VAL_SELF_LOOP,
//      GI_VAL_EMPTY).  A molecule with any of these bits gets an all-zero row, popcount 0, atom_id -1 and its status
//      word; nothing below is evaluated for it (so no diagonal bit is ever seen below).  deg_i and o2_i are taken from
//      that function's one pass over the rows (GiLabelledNode), not from a second walk with gi_atom_order2;
//   2  one thread per atom i < n: id_0[i] = mix64(K0 + a_i + 256 c_i + 2^16 deg_i + 2^24 o2_i);
//   3  rounds r = 1 .. R: id_r[i] = mix64(mix64(id_{r-1}[i] + r) + sum over bonds (t, j) of i of
//      mix64(id_{r-1}[j] ^ (K1 order2[t]))), 64-bit wrap-around (a commutative sum: no order to depend on), two [128]
//      arrays in LDS and a barrier between rounds;
//   4  after every round bit (id_r[i] & (n_bits - 1)) of the row in LDS is set (atomicOr); the row leaves in 16-byte
//      pieces (8 bytes when n_bits = 64).
// Integer arithmetic only; no global atomics, no scratch.  Every index is bounded by the dims: i, j < N because they
// come from an offset < N N Fe, a segment index < its segment's size because it comes from an offset < Fn and is used
// only when the row is one-hot, a bit index < n_bits <= 4096 by the mask.  Loops: Fe N words per atom and round,
// R <= 4 rounds.  LDS: Fe N 16 B dynamic (<= 16 KB), ~8 KB static.
//
// fp_compare_kernel  one 256-lane workgroup per tile of 16 query rows (<= 512 B each, in LDS):
//   lane l walks the set rows s = l, l + 256, ... in ascending order; a row is loaded once per workgroup with 16-byte
//   loads (8-byte ones when W = 2) and met with all 16 query rows (every lane reads the same LDS address: a broadcast);
//   b = popcount(s) is counted while loading.  Per pair c = popcount(q & s), u = a + b - c.
//   Nearest neighbour: the largest c / u, decided in integers (c1 u2 > c2 u1; ties to the lower s) — in the lane, then
//   across the wave's lanes (xor butterfly), then across the four waves.
//   SUMMATION ORDER of decision = intercept + sum_s weight[s] K(q, s), fp32, fixed, so the same inputs give the same
//   bits on every run: (1) each lane adds its terms in ascending s, starting from the first term; (2) the 64 lanes of a
//   wave are added by a 6-level xor butterfly (offsets 32, 16, .., 1; both partners compute the same sum); (3) the four
//   waves are added as ((w0 + w1) + w2) + w3; (4) the intercept is added last.  The longest chain of additions a term
//   goes through is k = ceil(S / 256) + 9 (ceil(S / 256) - 1 in the lane, 6, 3, 1).  The product weight[s] * K may be
//   fused into its addition; K itself is one fp32 division (Tanimoto), an exact integer (linear) or the fp64 exp
//   rounded once to fp32 (RBF).  proba = the Platt sigmoid of decision, evaluated in fp64 and rounded once; 0 where
//   a == 0.  No atomics anywhere.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int MAXW = GI_FP_MAX_BITS / 32;
constexpr int TILE = 16;                                     // query rows of a workgroup of fp_compare_kernel
constexpr int ZERO_ROW = GI_MOL_MALFORMED | GI_VAL_EMPTY | GI_VAL_SELF_LOOP;
constexpr u64 K0 = 0xD1B54A32D192ED03ull, K1 = 0x8CB92BA72F3D8DD7ull;

template <typename T>
__global__ __launch_bounds__(NT) void mol_fingerprint_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                             const void* __restrict__ n_nodes, int nn_bytes, int N,
                                                             int Fn, int Fe, int A, int C, int H,
                                                             const i8* __restrict__ order2, int radius, int W,
                                                             int* __restrict__ bits, int* __restrict__ popcount,
                                                             int* __restrict__ status, int* __restrict__ atom_id) {
    extern __shared__ unsigned adj[];                        // [Fe][N][4]: bit j of row (t, i): bond t between i and j
    __shared__ GiLabelled st;
    __shared__ u64 ids[2][MAXN];
    __shared__ __attribute__((aligned(16))) unsigned row[MAXW];
    __shared__ int pop_sh;
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    for (int i = tid; i < MAXW; i += NT) row[i] = 0u;
    if (tid == 0) pop_sh = 0;

    // ---- 1: read and check -------------------------------------------------------------------------------
    GiLabelledNode me;                                       // deg and o2 come from the pass that checks the rows
    const int n = gi_read_labelled<true>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes,
                                         nn_bytes, g, N, Fn, Fe, A, C, H, order2, tid, adj, st, nullptr, me);
    const bool sound = (st.flags & ZERO_ROW) == 0;           // uniform
    const bool mine = sound && tid < n;                      // this thread owns atom `tid`
    const unsigned fold_mask = (unsigned)(W * 32 - 1);

    // ---- 2-4: identifiers, rounds, folding (uniform control flow: every thread meets every barrier) ---------
    u64 id = 0;
    if (mine) {
        const int a = st.seg_first[0][tid], c = st.seg_first[1][tid];     // a < A, c < C: the row is one-hot
        id = mix64(K0 + (u64)a + 256ull * (u64)c + ((u64)me.deg << 16) + ((u64)me.o2 << 24));
        ids[0][tid] = id;
        const unsigned b = (unsigned)id & fold_mask;
        atomicOr(&row[b >> 5], 1u << (b & 31));
    }
    for (int r = 1; r <= radius; ++r) {
        __syncthreads();                                     // ids[(r - 1) & 1] is complete
        if (mine) {
            const u64* prev = ids[(r - 1) & 1];
            u64 sum = 0;
            for (int t = 0; t < Fe; ++t) {
                const u64 kt = K1 * (u64)order2[t];
                for (int w = 0; w < 4; ++w) {
                    unsigned nb = adj[(t * N + tid) * 4 + w];
                    while (nb) {
                        const int j = 32 * w + __builtin_ctz(nb);         // j < n <= N: the molecule is sound
                        nb &= nb - 1;
                        sum += mix64(prev[j] ^ kt);
                    }
                }
            }
            id = mix64(mix64(id + (u64)r) + sum);
            ids[r & 1][tid] = id;
            const unsigned b = (unsigned)id & fold_mask;
            atomicOr(&row[b >> 5], 1u << (b & 31));
        }
    }
    __syncthreads();

    // ---- outputs ---------------------------------------------------------------------------------------------
    if (tid < W && row[tid]) atomicAdd(&pop_sh, __popc(row[tid]));
    if (W >= 4) {
        if (tid < W / 4) reinterpret_cast<uint4*>(bits + (size_t)g * W)[tid] = reinterpret_cast<const uint4*>(row)[tid];
    } else if (tid == 0) {                                   // W == 2
        *reinterpret_cast<uint2*>(bits + (size_t)g * W) = *reinterpret_cast<const uint2*>(row);
    }
    if (atom_id)
        for (int a = tid; a < N; a += NT) {                  // N <= 128 < NT: thread a is atom a's owner
            int* o = atom_id + ((size_t)g * N + a) * 2;
            o[0] = mine ? (int)(unsigned)id : -1;
            o[1] = mine ? (int)(unsigned)(id >> 32) : -1;
        }
    __syncthreads();
    if (tid == 0) {
        popcount[g] = pop_sh;
        status[g] = st.flags;
    }
}

struct CmpOut {
    int* nearest;
    int* common;
    int* uni;
    float* max_sim;
    float* decision;
    float* proba;
};

// is (c1, u1, s1) the better neighbour: a larger c / u, or the same and a lower index
__device__ __forceinline__ bool fp_better(int c1, int u1, int s1, int c2, int u2, int s2) {
    const int l = c1 * u2, r = c2 * u1;                      // <= 4096 * 8192
    return l > r || (l == r && s1 < s2);
}

template <int V>                                             // words per load: 4, or 2 when W == 2
__global__ __launch_bounds__(NT) void fp_compare_kernel(const unsigned* __restrict__ query,
                                                        const unsigned* __restrict__ set,
                                                        const float* __restrict__ weight, int G, int S, int W, int kind,
                                                        double gamma, double intercept, double prob_a, double prob_b,
                                                        CmpOut out) {
    __shared__ __attribute__((aligned(16))) unsigned qt[TILE][MAXW];
    __shared__ int qa[TILE];
    __shared__ int red_c[NT / 64][TILE], red_u[NT / 64][TILE], red_s[NT / 64][TILE];
    __shared__ float red_f[NT / 64][TILE];
    const int tid = threadIdx.x, g0 = blockIdx.x * TILE;
    for (int idx = tid; idx < TILE * W; idx += NT) {
        const int q = idx / W, k = idx - q * W;
        qt[q][k] = g0 + q < G ? query[(size_t)(g0 + q) * W + k] : 0u;
    }
    __syncthreads();
    if (tid < TILE) {
        int a = 0;
        for (int k = 0; k < W; ++k) a += __popc(qt[tid][k]);
        qa[tid] = a;
    }
    __syncthreads();

    int cb[TILE], ub[TILE], sb[TILE];
    float acc[TILE];
#pragma unroll
    for (int q = 0; q < TILE; ++q) { cb[q] = 0; ub[q] = 1; sb[q] = 0x7fffffff; acc[q] = 0.f; }
    for (int s = tid; s < S; s += NT) {                      // ascending s in every lane
        int c[TILE];
#pragma unroll
        for (int q = 0; q < TILE; ++q) c[q] = 0;
        int b = 0;
        const unsigned* sr = set + (size_t)s * W;
        for (int k = 0; k < W; k += V) {
            unsigned x[V];
            if constexpr (V == 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(sr + k);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
                const uint2 v = *reinterpret_cast<const uint2*>(sr + k);
                x[0] = v.x; x[1] = v.y;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) b += __popc(x[e]);
#pragma unroll
            for (int q = 0; q < TILE; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) c[q] += __popc(x[e] & qt[q][k + e]);
        }
        const float w = weight ? weight[s] : 0.f;
#pragma unroll
        for (int q = 0; q < TILE; ++q) {
            const int a = qa[q], u = a + b - c[q];
            if (fp_better(c[q], u, s, cb[q], ub[q], sb[q])) { cb[q] = c[q]; ub[q] = u; sb[q] = s; }
            if (weight) {
                float K;
                if (kind == GI_FP_TANIMOTO) K = u > 0 ? (float)c[q] / (float)u : 0.f;
                else if (kind == GI_FP_RBF) K = (float)exp(-gamma * (double)(a + b - 2 * c[q]));
                else K = (float)c[q];
                acc[q] += w * K;                             // the lane's first term meets 0: exact
            }
        }
    }
#pragma unroll
    for (int q = 0; q < TILE; ++q) {                         // the wave's lanes: a 6-level xor butterfly
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oc = __shfl_xor(cb[q], off), ou = __shfl_xor(ub[q], off), os = __shfl_xor(sb[q], off);
            if (fp_better(oc, ou, os, cb[q], ub[q], sb[q])) { cb[q] = oc; ub[q] = ou; sb[q] = os; }
            acc[q] += __shfl_xor(acc[q], off);
        }
        if ((tid & 63) == 0) {
            red_c[tid >> 6][q] = cb[q]; red_u[tid >> 6][q] = ub[q]; red_s[tid >> 6][q] = sb[q];
            red_f[tid >> 6][q] = acc[q];
        }
    }
    __syncthreads();
    if (tid < TILE && g0 + tid < G) {                        // the four waves, in order
        const int g = g0 + tid, a = qa[tid];
        int c = red_c[0][tid], u = red_u[0][tid], s = red_s[0][tid];
        float f = red_f[0][tid];
        for (int w = 1; w < NT / 64; ++w) {
            if (fp_better(red_c[w][tid], red_u[w][tid], red_s[w][tid], c, u, s)) {
                c = red_c[w][tid]; u = red_u[w][tid]; s = red_s[w][tid];
            }
            f += red_f[w][tid];
        }
        const bool live = a > 0;                             // then u >= a > 0
        out.nearest[g] = live ? s : -1;
        out.common[g] = live ? c : 0;
        out.uni[g] = live ? u : 0;
        out.max_sim[g] = live ? (float)c / (float)u : 0.f;
        if (weight) {
            f += (float)intercept;
            out.decision[g] = f;
            const double t = prob_a * (double)f + prob_b, e = exp(-fabs(t));
            out.proba[g] = live ? (float)(t >= 0. ? e / (1. + e) : 1. / (1. + e)) : 0.f;
        }
    }
}

bool fp_width_ok(int W) { return W >= GI_FP_MIN_BITS / 32 && W <= MAXW && (W & (W - 1)) == 0; }

}  // namespace

extern "C" int gi_mol_fingerprint(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                                  const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                                  const signed char* order2, int radius, int n_bits, int* bits, int* popcount,
                                  int* status, int* atom_id, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if (radius < 0 || radius > GI_FP_MAX_RADIUS || n_bits % 32 != 0 || !fp_width_ok(n_bits / 32)) return GI_EINVAL;
    if (G == 0) return 0;
    if (!nodes || !edges || !order2 || !bits || !popcount || !status || ((uintptr_t)bits & 15)) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned);                                      // <= 16 KB
    const int W = n_bits / 32;
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_fingerprint_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2,
                           radius, W, bits, popcount, status, atom_id);
    else
        hipLaunchKernelGGL(mol_fingerprint_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2, radius, W, bits,
                           popcount, status, atom_id);
    return gi_launch_status();
}

extern "C" int gi_fp_compare(int G, int S, int W_query, int W_set, const int* query, const int* set,
                             const float* weight, int kind, double gamma, double intercept, double prob_a,
                             double prob_b, int* nearest, int* common, int* uni, float* max_sim, float* decision,
                             float* proba, void* stream) {
    (void)hipGetLastError();
    if (G < 0 || S < 1 || W_query != W_set || !fp_width_ok(W_set)) return GI_EINVAL;
    if (kind != GI_FP_TANIMOTO && kind != GI_FP_RBF && kind != GI_FP_LINEAR) return GI_EINVAL;
    if (G == 0) return 0;
    if (!query || !set || !nearest || !common || !uni || !max_sim || (weight && (!decision || !proba)) ||
        (((uintptr_t)query | (uintptr_t)set) & 15))
        return GI_EINVAL;
    const CmpOut out = {nearest, common, uni, max_sim, decision, proba};
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(gi_cdiv(G, TILE));
    if (W_set >= 4)
        hipLaunchKernelGGL(fp_compare_kernel<4>, grid, dim3(NT), 0, st, (const unsigned*)query, (const unsigned*)set,
                           weight, G, S, W_set, kind, gamma, intercept, prob_a, prob_b, out);
    else
        hipLaunchKernelGGL(fp_compare_kernel<2>, grid, dim3(NT), 0, st, (const unsigned*)query, (const unsigned*)set,
                           weight, G, S, W_set, kind, gamma, intercept, prob_a, prob_b, out);
    return gi_launch_status();
}
