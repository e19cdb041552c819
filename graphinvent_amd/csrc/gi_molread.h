// Molecule I/O of the kernels that take a whole molecule (nodes [G, N, Fn] / edges [G, N, N, Fe], fp32 or int8), one
// 256-lane workgroup per molecule: gi_analyze.hip, gi_canon.hip, gi_reorder.hip (readers without segments, with their
// own error vocabularies), gi_valence.hip, gi_fingerprint.hip, gi_smiles.hip (the labelled read below), gi_smiles_read.hip
// (store_bytes, the valence helpers and the tables it shares with the writer) and the hash and wave helpers of
// gi_route.hip.  Here, once each:
//   the granule reader   every byte of p[0, len) is read once, at any element alignment: whole 16-byte granules of the
//                        ADDRESS range in one load, a ragged first or last granule element by element, nothing outside
//                        p[0, len) touched (gi_granule_count / gi_load_granule, gi_for_each_nonzero on top of them);
//   store_bytes          the same split for writing an int8 [D0, D1, D2] array;
//   gi_mol_structure     n (given or derived) and the GI_MOL_* structure bits from the adjacency rows in LDS;
//   gi_read_labelled     stages 1-2 of the kernels that judge a labelled molecule: the read, the segment counts, the
//                        structure check and the GI_MOL_MALFORMED / self-loop / empty bits, state in a GiLabelled (LDS)
//                        and a GiLabelledNode (the lane's registers);
//   gi_atom_order2, gi_hydrogen_fill   an atom's bond-order sum and the hydrogens up to its next allowed valence;
//   organic_valences, row_bit          what the SMILES writer and reader must share to stay inverses;
//   mix64, the wave reductions, gi_is01, gi_load_count, gi_below_word, and the host-side argument checks.
#pragma once
#include "gi_common.h"

constexpr int GI_MOL_NT = 256;                               // lanes of a workgroup that reads a molecule

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {      // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += (unsigned long long)__shfl_xor((long long)x, s);
    return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x = max(x, __shfl_xor(x, s));
    return x;
}

__device__ __forceinline__ bool gi_is01(float x) { return x == 0.f || x == 1.f; }
__device__ __forceinline__ bool gi_is01(signed char x) { return x == 0 || x == 1; }

__device__ __forceinline__ long long gi_load_count(const void* p, int bytes, long long g) {
    return bytes == 1 ? (long long)((const signed char*)p)[g] : bytes == 4 ? (long long)((const int*)p)[g]
                                                                           : ((const long long*)p)[g];
}

// bits [0, k) set, 0 <= k <= 128, as four 32-bit words
__device__ __forceinline__ unsigned gi_below_word(int k, int w) {
    const int r = k - 32 * w;
    return r <= 0 ? 0u : r >= 32 ? ~0u : (1u << r) - 1u;
}

// 16-byte granules of the address range that p[0, len) occupies
template <typename T>
__device__ __forceinline__ int gi_granule_count(const T* p, int len) {
    constexpr int E = 16 / (int)sizeof(T);
    return ((int)(((uintptr_t)p & 15) / sizeof(T)) + len + E - 1) / E;
}

// the elements of p[0, len) inside granule q: v[0, c) = p[o0, o0 + c), v[c, E) = 0, c returned.  A whole granule is one
// 16-byte load, a ragged first or last one is read element by element: nothing outside p[0, len) is touched.
template <typename T>
__device__ __forceinline__ int gi_load_granule(const T* p, int len, int q, int& o0, T (&v)[16 / sizeof(T)]) {
    constexpr int E = 16 / (int)sizeof(T);
    const int lo = q * E - (int)(((uintptr_t)p & 15) / sizeof(T));
    const int a = max(lo, 0), b = min(lo + E, len);
    o0 = a;
    if (b - a == E) {
        const uint4 w = *reinterpret_cast<const uint4*>(p + a);
        __builtin_memcpy(v, &w, 16);
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = k < b - a ? p[a + k] : (T)0;
    }
    return b - a;
}

// f(offset, value) for every non-zero element of p[0, len), the workgroup's lanes striding over the granules
template <typename T, class F>
__device__ __forceinline__ void gi_for_each_nonzero(const T* p, int len, int tid, F f) {
    constexpr int E = 16 / (int)sizeof(T);
    const int P = gi_granule_count(p, len);
    for (int q = tid; q < P; q += GI_MOL_NT) {
        T v[E];
        int o0;
        const int c = gi_load_granule(p, len, q, o0, v);
        uint4 w;
        __builtin_memcpy(&w, v, 16);
        if ((w.x | w.y | w.z | w.w) == 0) continue;         // molecules are mostly zeros (+0.f is all zero bits)
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (k < c && !(v[k] == (T)0)) f(o0 + k, v[k]);
    }
}

// bytes [0, len) at `p`, a [D0, D1, D2] array, written in 16-byte pieces between the ragged ends of the address range:
// src(a, b) names the source of the D2 bytes of pair (a, b) (negative: zeros) and is evaluated once per pair and piece,
// val(s, t) is byte t of source s
template <class S, class V>
__device__ __forceinline__ void store_bytes(signed char* p, int len, int tid, int D0, int D1, int D2, S src, V val) {
    const int head = min(len, (int)((16 - ((uintptr_t)p & 15)) & 15));
    const int pieces = (len - head) >> 4, tail0 = head + (pieces << 4);
    auto one = [&](int o) {
        const int e = o / D2, a = e / D1, s = src(a, e - a * D1);
        p[o] = (signed char)(s < 0 ? 0 : val(s, o - e * D2));
    };
    for (int o = tid; o < head; o += GI_MOL_NT) one(o);
    for (int o = tail0 + tid; o < len; o += GI_MOL_NT) one(o);
    for (int q = tid; q < pieces; q += GI_MOL_NT) {
        const int o = head + (q << 4);
        const int e = o / D2;
        int t = o - e * D2, a = e / D1, b = e - a * D1;
        int s = src(a, b);
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (s >= 0) w[k >> 2] |= (unsigned)(val(s, t) & 0xff) << ((k & 3) * 8);
            if (++t == D2) {
                t = 0;
                if (++b == D1) { b = 0; ++a; }
                s = a < D0 ? src(a, b) : -1;                 // a == D0: the piece ends with the array
            }
        }
        *reinterpret_cast<uint4*>(p + o) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The structure check of a molecule whose rows are complete in LDS (call it behind the barrier that ends the reading):
// adj [Fe][N][4], bit j of row (t, i) = bond t between i and j; present, bit i = node row i has a set entry.  Returns
// n: n_nodes[g] clamped to [0, N], or without n_nodes the number of LEADING rows with a set entry.  ORs into `err`
// GI_MOL_NODE_PAST_N (n_nodes[g] outside [0, N], or a set entry in a row >= n), GI_MOL_BOND_PAST_N (a bond that touches
// a node >= n) and GI_MOL_ASYMMETRIC (bond t from i to j without its mirror image), each in some lane of the workgroup.
__device__ __forceinline__ int gi_mol_structure(const unsigned* adj, const unsigned* present, const void* n_nodes,
                                                int nn_bytes, int g, int N, int Fe, int tid, int& err) {
    int n;
    if (n_nodes) {
        const long long c = gi_load_count(n_nodes, nn_bytes, g);
        if (c < 0 || c > N) err |= GI_MOL_NODE_PAST_N;
        n = (int)(c < 0 ? 0 : c > N ? N : c);
    } else {
        n = 0;
        while (n < 4 && present[n] == ~0u) ++n;
        n = n == 4 ? 128 : 32 * n + __builtin_ctz(~present[n]);
    }
    if (tid < 4 && (present[tid] & ~gi_below_word(n, tid))) err |= GI_MOL_NODE_PAST_N;
    for (int idx = tid; idx < Fe * N; idx += GI_MOL_NT) {    // row (t, i): inside n, and mirrored
        const int t = idx / N, i = idx - t * N;
        for (int w = 0; w < 4; ++w) {
            unsigned bits = adj[idx * 4 + w];
            if (bits == 0) continue;
            if (i >= n || (bits & ~gi_below_word(n, w))) err |= GI_MOL_BOND_PAST_N;
            while (bits) {
                const int b = __builtin_ctz(bits), j = 32 * w + b;         // j < N: it came from an offset < N N Fe
                bits &= bits - 1;
                if (!((adj[(t * N + j) * 4 + (i >> 5)] >> (i & 31)) & 1u)) err |= GI_MOL_ASYMMETRIC;
            }
        }
    }
    return n;
}

// ---- the labelled read: a molecule whose node rows have segments (atom type | formal charge | implicit H | ignored) ----
// The bits that make a molecule malformed: gi_mol_valence's verdict, gi_mol_fingerprint's zero row and gi_mol_smiles'
// empty string agree on them because all three get them from gi_read_labelled.
constexpr int GI_MOL_MALFORMED = GI_MOL_ONEHOT | GI_MOL_BOND_PAST_N | GI_MOL_VALUE | GI_MOL_MULTI_BOND |
                                 GI_MOL_ASYMMETRIC | GI_MOL_NODE_PAST_N;
constexpr int GI_LABEL_EMPTY = 128, GI_LABEL_SELF_LOOP = 256;            // under both names of the public header
static_assert(GI_VAL_EMPTY == GI_LABEL_EMPTY && GI_SMI_EMPTY == GI_LABEL_EMPTY, "one empty bit");
static_assert(GI_VAL_SELF_LOOP == GI_LABEL_SELF_LOOP && GI_SMI_SELF_LOOP == GI_LABEL_SELF_LOOP, "one self-loop bit");

// What a labelled read leaves in (static) LDS: per node and segment the number of set entries and the lowest of them
// (relative to the segment; 0x7fffffff: none), the node rows with a set entry, the workgroup's status bits.
struct GiLabelled {
    int seg_cnt[3][GI_MAX_NODES], seg_first[3][GI_MAX_NODES];
    unsigned present[4];
    int flags;
};

// What the read leaves in the registers of the lane that owns node `tid` (zeros for tid >= N): the OR over the bond
// types of the node's rows, whether it has a bond of order 1.5, and, where the caller asks for them (DEG_O2), the number
// of its bonded partners and twice its bond-order sum (gi_atom_order2), counted in the same pass over the rows.
struct GiLabelledNode {
    unsigned seen[4];
    int deg, o2;
    bool arom;
};

// Reads molecule g once and checks it.  The CALLER has zeroed adj [Fe][N][4] (and whatever else it owns) and has NOT yet
// met a barrier; `st` is cleared here.  Three barriers: behind the clearing, behind the reading, behind the publishing
// of the bits; after the last one st.flags is uniform and holds GI_MOL_VALUE, the bits of gi_mol_structure, _ONEHOT,
// _MULTI_BOND, GI_LABEL_SELF_LOOP and GI_LABEL_EMPTY.  A, C, H: the segment sizes, A + C + H <= Fn (checked on the
// host); what follows them in a node row (a chirality segment) is not looked at.  Returns n.  `orr` (LDS [N][4], or
// nullptr): me.seen of every node, stored in front of the last barrier.  Every index is bounded by the dims: i, j < N
// from an offset < N N Fe, a segment index < its size from an offset < Fn.
template <bool DEG_O2, typename T>
__device__ __forceinline__ int gi_read_labelled(const T* nd, const T* ed, const void* n_nodes, int nn_bytes, int g,
                                                int N, int Fn, int Fe, int A, int C, int H, const signed char* order2,
                                                int tid, unsigned* adj, GiLabelled& st, unsigned (*orr)[4],
                                                GiLabelledNode& me) {
    const int o_c = A, o_h = A + C, o_x = A + C + H;         // segment ends
    for (int i = tid; i < 3 * GI_MAX_NODES; i += GI_MOL_NT) {
        (&st.seg_cnt[0][0])[i] = 0;
        (&st.seg_first[0][0])[i] = 0x7fffffff;
    }
    if (tid < 4) st.present[tid] = 0u;
    if (tid == 0) st.flags = 0;
    __syncthreads();
    int flags = 0;
    gi_for_each_nonzero(nd, N * Fn, tid, [&](int o, T v) {
        if (!gi_is01(v)) flags |= GI_MOL_VALUE;
        const int i = o / Fn, f = o - i * Fn;                // i < N
        atomicOr(&st.present[i >> 5], 1u << (i & 31));
        if (f < o_x) {
            const int s = f < o_c ? 0 : f < o_h ? 1 : 2;
            atomicAdd(&st.seg_cnt[s][i], 1);
            atomicMin(&st.seg_first[s][i], f - (s == 0 ? 0 : s == 1 ? o_c : o_h));
        }
    });
    gi_for_each_nonzero(ed, N * N * Fe, tid, [&](int o, T v) {
        if (!gi_is01(v)) flags |= GI_MOL_VALUE;
        const int e = o / Fe, t = o - e * Fe, i = e / N, j = e - i * N;
        if (i == j) flags |= GI_LABEL_SELF_LOOP;
        atomicOr(&adj[(t * N + i) * 4 + (j >> 5)], 1u << (j & 31));
    });
    __syncthreads();
    const int n = gi_mol_structure(adj, st.present, n_nodes, nn_bytes, g, N, Fe, tid, flags);
    me.arom = false;
    me.deg = me.o2 = 0;
    for (int w = 0; w < 4; ++w) me.seen[w] = 0u;
    if (tid < N) {                                           // this lane's node: several types on a pair, one-hot segments
        for (int t = 0; t < Fe; ++t) {
            int cnt = 0;
            for (int w = 0; w < 4; ++w) {
                const unsigned row = adj[(t * N + tid) * 4 + w];
                const unsigned diag = (tid >> 5) == w ? 1u << (tid & 31) : 0u;
                if (row & me.seen[w] & ~diag) flags |= GI_MOL_MULTI_BOND;
                if (row && order2[t] == 3) me.arom = true;
                me.seen[w] |= row;
                if constexpr (DEG_O2) cnt += __popc(row);
            }
            if constexpr (DEG_O2) me.o2 += (int)order2[t] * cnt;         // <= 6 * 8 * 128
        }
        if constexpr (DEG_O2)
            for (int w = 0; w < 4; ++w) me.deg += __popc(me.seen[w]);
        if (orr)
            for (int w = 0; w < 4; ++w) orr[tid][w] = me.seen[w];
        if (tid < n && (st.seg_cnt[0][tid] != 1 || st.seg_cnt[1][tid] != 1 || (H > 0 && st.seg_cnt[2][tid] != 1)))
            flags |= GI_MOL_ONEHOT;
    }
    if (n == 0) flags |= GI_LABEL_EMPTY;
    if (flags) atomicOr(&st.flags, flags);
    __syncthreads();
    return n;
}

// twice the bond-order sum of atom i: sum over bond types of order2[t] * popcount(row (t, i)), <= 6 * 8 * 128
__device__ __forceinline__ int gi_atom_order2(const unsigned* adj, const signed char* order2, int N, int Fe, int i) {
    int o2 = 0;
    for (int t = 0; t < Fe; ++t) {
        int deg = 0;
        for (int w = 0; w < 4; ++w) deg += __popc(adj[(t * N + i) * 4 + w]);
        o2 += (int)order2[t] * deg;
    }
    return o2;
}

// the hydrogens that take an atom of valence x to the lowest allowed valence >= x (bit v of `allowed` = total valence
// v, v <= 15); -1: there is none, the atom is over its valence
__device__ __forceinline__ int gi_hydrogen_fill(unsigned allowed, int x) {
    const unsigned at_least = x > 15 ? 0u : (allowed >> x) << x;
    return at_least ? __builtin_ctz(at_least) - x : -1;
}

// the normal valences of the OpenSMILES organic subset as a bit mask (bit v), 0 for any other symbol: ONE table for the
// writer (gi_smiles.hip) and the reader (gi_smiles_read.hip), which is the writer's inverse
__device__ __forceinline__ unsigned organic_valences(unsigned char s0, unsigned char s1) {
    if (s1 == 0) {
        switch (s0) {
            case 'B': return 1u << 3;
            case 'C': return 1u << 4;
            case 'N': case 'P': return (1u << 3) | (1u << 5);
            case 'O': return 1u << 2;
            case 'S': return (1u << 2) | (1u << 4) | (1u << 6);
            case 'F': case 'I': return 1u << 1;
            default: return 0u;
        }
    }
    return ((s0 == 'C' && s1 == 'l') || (s0 == 'B' && s1 == 'r')) ? 1u << 1 : 0u;
}

__device__ __forceinline__ bool row_bit(const unsigned* row, int j) { return (row[j >> 5] >> (j & 31)) & 1u; }

// The argument checks common to the gi_mol_* and gi_smiles_* entry points, in parts because the entry points order
// them differently and the first that fires decides the code: the dims and limits ...
static inline int gi_mol_check_dims(int G, int N, int Fn, int Fe) {
    if (G < 0 || N < 1 || Fn < 1 || Fe < 1 || N > GI_MAX_NODES || Fe > GI_MAX_GROUPS) return GI_EINVAL;
    if (Fn > GI_ANALYZE_MAX_FN) return GI_ELIMIT;
    return 0;
}
// ... the molecules' dtype and the width of an n_nodes entry ...
static inline int gi_mol_check_types(int dtype, int nn_bytes) {
    if ((dtype != GI_DTYPE_F32 && dtype != GI_DTYPE_I8) || (nn_bytes != 1 && nn_bytes != 4 && nn_bytes != 8))
        return GI_EINVAL;
    return 0;
}
// ... the segments of a labelled node row ...
static inline int gi_mol_check_segments(int n_types, int n_charges, int n_imp_h, int Fn) {
    if (n_types < 1 || n_charges < 1 || n_imp_h < 0 || (long long)n_types + n_charges + n_imp_h > Fn) return GI_EINVAL;
    return 0;
}
// ... and the row pitch of a batch of strings
static inline int gi_smi_check_max_len(int max_len) {
    if (max_len < 16 || (max_len & 15)) return GI_EINVAL;
    if (max_len > GI_SMI_MAX_LEN) return GI_ELIMIT;
    return 0;
}
