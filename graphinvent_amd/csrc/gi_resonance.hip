// The resonance normal form on the device (gfx950): which bonds of a molecule change order between its Kekule
// structures (gi_mol_resonance), and the inverse, one Kekule structure chosen as a function of the indexed graph
// (gi_mol_kekulize).  THIS IS NOT AROMATICITY PERCEPTION: no Hueckel count, no chemistry table, no moving charges, no
// tautomers; cyclobutadiene and cyclooctatetraene are delocalised, pyrrole and furan are not (they have one Kekule
// structure, identity needs nothing there).  The rule is written out in include/graphinvent_amd.h at
// gi_mol_resonance; tests/resonance_model.py is the specification, matched integer for integer.
//
// mol_resonance_kernel  one 256-lane WORKGROUP per molecule:
//   1, 2  gi_read_labelled of gi_molread.h (the front end of gi_valence.hip): every byte read once in 16-byte pieces
//      (fp32 or int8, any alignment) into one 128-bit adjacency row per (bond type, node) in LDS; n given or derived; the
//      GI_MOL_MALFORMED / self-loop / empty bits (any of them: nothing is delocalised, the edges are copied);
//   3  one lane per atom: d (order-2 bonds), t (order-3 and order-1.5 bonds), its double-bond partner; a ballot builds
//      the V' mask (d = 1, t = 0, and the partner too), then the rows of G' (single or double bonds inside V') and
//      `mate`, the perfect matching M the double bonds are;
//   4  the verdicts, by augmenting-path searches with blossom contraction (gi_res_search.h, host-device code that also
//      runs on the host against the specification).  SLOTS = 64 lanes search at once, 16 in each wave so that the four
//      SIMDs share the divergent work; slot s owns atoms s and s + 64.  First the double bonds (a, mate a), a < mate a:
//      delocalised iff a path joins a and mate a in G' - e.  Behind a barrier the single bonds (u, v) whose ends both sit
//      on a delocalised double bond: delocalised iff a path joins mate u and mate v in G' - u - v.  A successful search
//      closes an alternating cycle and marks ALL its bonds (LDS atomicOr); a bond found marked is not searched again.
//      The verdict is definitional, so the order in which lanes find the cycles does not show in the result.
//      Each slot has private parent / base / queue bytes in LDS ([3][N][SLOTS], entry k of slot s at k * SLOTS + s) and
//      its used / blossom / seen masks in registers;
//   5  one lane per atom again: the counts, the components of the delocalised bonds by min-label propagation (at most
//      n rounds), the 128-bit rows, and the normal form [N, N, Fe + 1] written in 16-byte pieces (store_bytes): the
//      rows are copied, a delocalised bond moves to channel Fe.
// mol_kekulize_kernel  the same front end on Fe + 1 channels; ONE lane runs `match` on the channel-Fe rows exactly as
//      the SMILES reader's kekuliser does (greedy in ascending index, then one search per free atom, neighbours
//      ascending), all lanes write the Fe-channel edges.
// Integers only, no global atomics, no scratch memory, nothing to clear in front of a launch.  Every loop is bounded by
// N or by the number of G' bonds.  Every index is bounded by the dims: atoms < n <= N come out of rows cut to n, and
// gi_res_search.h compares every index it reads back from its workspace with n.
// LDS of mol_resonance_kernel: 9.9 KB static (three [128][4] row sets, GiLabelled, mate, labels) and Fe N 16 + 3 N 64
// bytes dynamic: 13.3 KB at N = 13, 27.5 KB at N = 72 and Fe = 3, 51.1 KB at the limits (N = 128, Fe = 8), which keeps
// three workgroups on a CU (160 KB) and needs no raised dynamic limit.  128 slots would halve the tail of a search-bound
// molecule and cost 24 KB more: two workgroups per CU for the read, which every molecule pays.
#include "gi_common.h"
#include "gi_molread.h"
#include "gi_res_search.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int SLOTS = 64, SLOT_LANES = SLOTS / (NT / 64);    // searching lanes of a workgroup / of a wave
constexpr int UNSOUND = GI_MOL_MALFORMED | GI_LABEL_EMPTY | GI_LABEL_SELF_LOOP;
static_assert(GI_RES_EMPTY == GI_LABEL_EMPTY && GI_RES_SELF_LOOP == GI_LABEL_SELF_LOOP, "one empty, one self-loop bit");
static_assert(MAXN <= RES_NONE, "an atom index fits a byte beside RES_NONE");

struct ResOut {
    int *status, *n_delocalized, *n_atoms, *n_systems, *delocalized;
    i8* edges;
};

// the delocalised bonds as 128-bit rows in LDS, marked by any lane at any time
struct LdsMarks {
    unsigned (*row)[4];
    __device__ __forceinline__ void mark(int a, int b) {
        atomicOr(&row[a][b >> 5], 1u << (b & 31));
        atomicOr(&row[b][a >> 5], 1u << (a & 31));
    }
    __device__ __forceinline__ bool marked(int a, int b) const {
        return (((volatile const unsigned*)row[a])[b >> 5] >> (b & 31)) & 1u;
    }
};

template <typename T>
__global__ __launch_bounds__(NT) void mol_resonance_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                           const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                           int Fe, int A, int C, int H, const i8* __restrict__ order2,
                                                           ResOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* adj = reinterpret_cast<unsigned*>(smem);       // [Fe][N][4]: bit j of row (t, i): bond t between i and j
    unsigned char* ws = smem + (size_t)Fe * N * 16;          // [3][N][SLOTS]: parent, base, queue of every slot
    __shared__ unsigned orr[MAXN][4];                        // the OR of a node's rows over the bond types
    __shared__ unsigned gp[MAXN][4];                         // its row in G'
    __shared__ unsigned del[MAXN][4];                        // its delocalised bonds
    __shared__ GiLabelled st;
    __shared__ unsigned vmask[4];
    __shared__ int comp[MAXN], sums[3], info;                // sums: set bits of del, atoms, systems
    __shared__ unsigned char mate[MAXN];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    for (int i = tid; i < MAXN * 4; i += NT) (&del[0][0])[i] = 0u;
    if (tid < 3) sums[tid] = 0;
    if (tid == 0) info = 0;

    // ---- 1, 2: read and check ---------------------------------------------------------------------------------
    GiLabelledNode me;
    const int n = gi_read_labelled<false>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes,
                                          nn_bytes, g, N, Fn, Fe, A, C, H, order2, tid, adj, st, orr, me);
    const bool sound = (st.flags & UNSOUND) == 0;            // uniform

    if (sound) {
        // ---- 3: V', G' and M ------------------------------------------------------------------------------------
        unsigned d4[4] = {0u, 0u, 0u, 0u}, s4[4] = {0u, 0u, 0u, 0u};
        bool ok = false;
        int partner = RES_NONE;
        if (tid < n) {
            int d = 0, t3 = 0;
            for (int t = 0; t < Fe; ++t) {
                const int o = order2[t];
                for (int w = 0; w < 4; ++w) {
                    const unsigned row = adj[(t * N + tid) * 4 + w];
                    if (o == 4) { d4[w] |= row; d += __popc(row); }
                    else if (o == 2) s4[w] |= row;
                    else if (o == 6 || o == 3) t3 += __popc(row);
                }
            }
            ok = d == 1 && t3 == 0;
            if (me.arom) atomicOr(&info, GI_RES_AROMATIC);   // informational: a stored order-1.5 bond
            if (ok) partner = d4[0] ? __builtin_ctz(d4[0]) : d4[1] ? 32 + __builtin_ctz(d4[1])
                                    : d4[2] ? 64 + __builtin_ctz(d4[2]) : 96 + __builtin_ctz(d4[3]);      // < n: sound
        }
        if (tid < MAXN) mate[tid] = (unsigned char)partner;  // RES_NONE: not a candidate
        __syncthreads();
        const bool in_v = ok && mate[partner] != RES_NONE;   // the partner is a candidate too (its partner is this atom)
        const u64 vb = __ballot(in_v);
        if (lane == 0 && wave < 2) {                         // atoms 0 .. 127 are the lanes of waves 0 and 1
            vmask[2 * wave] = (unsigned)vb;
            vmask[2 * wave + 1] = (unsigned)(vb >> 32);
        }
        __syncthreads();                                     // every mate[partner] has been read
        if (tid < MAXN) {
            if (!in_v) mate[tid] = (unsigned char)RES_NONE;
            for (int w = 0; w < 4; ++w) gp[tid][w] = in_v ? (d4[w] | s4[w]) & vmask[w] : 0u;
        }
        __syncthreads();

        // ---- 4: the verdicts --------------------------------------------------------------------------------------
        LdsMarks marks = {del};
        const bool searcher = lane < SLOT_LANES;
        const int slot = wave * SLOT_LANES + lane;           // < SLOTS for a searcher
        unsigned char* parent = ws + slot;
        unsigned char* base = parent + N * SLOTS;
        unsigned char* queue = base + N * SLOTS;
        if (searcher)
            for (int a = slot; a < n; a += SLOTS) res_doubles(&gp[0][0], n, mate, a, parent, base, queue, SLOTS, marks);
        __syncthreads();                                     // the double bonds are decided
        if (searcher)
            for (int u = slot; u < n; u += SLOTS) res_singles(&gp[0][0], n, mate, u, parent, base, queue, SLOTS, marks);
        __syncthreads();

        // ---- 5: counts and components -----------------------------------------------------------------------------
        int bits = 0;
        if (tid < n)
            for (int w = 0; w < 4; ++w) bits += __popc(del[tid][w]);
        const bool on = bits > 0;
        if (tid < MAXN) comp[tid] = tid;
        if (on) { atomicAdd(&sums[0], bits); atomicAdd(&sums[1], 1); }
        __syncthreads();
        for (int round = 0; round < n; ++round) {            // uniform: the exit is a workgroup-wide vote
            int m = MAXN;
            if (on) {
                m = comp[tid];
                for (int w = 0; w < 4; ++w) {
                    unsigned r = del[tid][w];
                    while (r) {
                        m = min(m, comp[32 * w + __builtin_ctz(r)]);     // < n: a marked atom
                        r &= r - 1;
                    }
                }
            }
            const bool changed = on && m < comp[tid];
            __syncthreads();                                 // every label of this round has been read
            if (changed) comp[tid] = m;
            if (!__syncthreads_or(changed)) break;
        }
        if (on && comp[tid] == tid) atomicAdd(&sums[2], 1);
        __syncthreads();
    }

    // ---- outputs -----------------------------------------------------------------------------------------------
    if (tid < N)
        for (int w = 0; w < 4; ++w) out.delocalized[((size_t)g * N + tid) * 4 + w] = (int)del[tid][w];
    if (tid == 0) {
        out.status[g] = st.flags | info;
        out.n_delocalized[g] = sums[0] >> 1;
        out.n_atoms[g] = sums[1];
        out.n_systems[g] = sums[2];
    }
    if (out.edges) {
        const int one = (st.flags & GI_MOL_VALUE) ? 2 : 1;   // a molecule with an entry that is not 0 / 1 keeps one
        const int D2 = Fe + 1;
        store_bytes(out.edges + (size_t)g * (N * N * D2), N * N * D2, tid, N, N, D2,
                    [&](int a, int b) { return row_bit(orr[a], b) ? a * MAXN + b : -1; },
                    [&](int s, int t) {
                        const int i = s / MAXN, j = s - i * MAXN;
                        const bool dl = row_bit(del[i], j);
                        if (t == Fe) return dl ? 1 : 0;
                        return !dl && row_bit(adj + (t * N + i) * 4, j) ? one : 0;
                    });
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void mol_kekulize_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                          const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                          int Fe, int A, int C, int H, const i8* __restrict__ order2,
                                                          int* __restrict__ status, i8* __restrict__ edges_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* adj = reinterpret_cast<unsigned*>(smem);       // [Fe + 1][N][4]; channel Fe: the delocalised bonds
    __shared__ unsigned orr[MAXN][4];
    __shared__ GiLabelled st;
    __shared__ unsigned char mate[MAXN], parent[MAXN], base[MAXN], queue[MAXN];
    __shared__ i8 o2x[GI_MAX_GROUPS];
    __shared__ int kflags;
    const int g = blockIdx.x, tid = threadIdx.x, Fi = Fe + 1;
    for (int i = tid; i < Fi * N * 4; i += NT) adj[i] = 0u;
    if (tid < Fi) o2x[tid] = tid < Fe ? order2[tid] : (i8)0;  // channel Fe has no order of its own
    if (tid == 0) kflags = 0;

    GiLabelledNode me;
    const int n = gi_read_labelled<false>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fi), n_nodes,
                                          nn_bytes, g, N, Fn, Fi, A, C, H, o2x, tid, adj, st, orr, me);
    const bool sound = (st.flags & UNSOUND) == 0;            // uniform
    int single = -1, dbl = -1;
    for (int t = Fe - 1; t >= 0; --t) {                      // the FIRST type of each order
        if (order2[t] == 2) single = t;
        if (order2[t] == 4) dbl = t;
    }
    const unsigned* marked = adj + Fe * N * 4;               // [N][4]
    if (sound) {
        if (me.arom) atomicOr(&kflags, GI_RES_AROMATIC);
        if (tid == 0) {                                      // ONE lane, as in the reader: the choice follows the indices
            bool any = false;
            for (int i = 0; i < n * 4; ++i) any |= marked[i] != 0u;
            int flags = 0;
            if (any && (single < 0 || dbl < 0)) flags |= GI_RES_BOND_ORDER;
            if (!res_match(marked, n, mate, parent, base, queue, nullptr)) flags |= GI_RES_NO_KEKULE;
            if (flags) atomicOr(&kflags, flags);
        }
    }
    __syncthreads();
    const int flags = st.flags | kflags;
    const bool bad = (flags & (UNSOUND | GI_RES_BOND_ORDER | GI_RES_NO_KEKULE)) != 0;
    if (tid == 0) status[g] = flags;
    store_bytes(edges_out + (size_t)g * (N * N * Fe), N * N * Fe, tid, N, N, Fe,
                [&](int a, int b) { return !bad && row_bit(orr[a], b) ? a * MAXN + b : -1; },
                [&](int s, int t) {
                    const int i = s / MAXN, j = s - i * MAXN;
                    if (row_bit(marked + i * 4, j)) return t == ((int)mate[i] == j ? dbl : single) ? 1 : 0;
                    return row_bit(adj + (t * N + i) * 4, j) ? 1 : 0;
                });
}

}  // namespace

extern "C" int gi_mol_resonance(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                                const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                                const signed char* order2, int* status, int* n_delocalized, int* n_atoms, int* n_systems,
                                int* delocalized, signed char* edges_out, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if (edges_out && Fe + 1 > GI_MAX_GROUPS) return GI_ELIMIT;               // the normal form has one channel more
    if (G == 0) return 0;
    if (!nodes || !edges || !order2 || !status || !n_delocalized || !n_atoms || !n_systems || !delocalized)
        return GI_EINVAL;
    const ResOut out = {status, n_delocalized, n_atoms, n_systems, delocalized, edges_out};
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 16 + (size_t)3 * N * SLOTS;                                // <= 40 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_resonance_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2,
                           out);
    else
        hipLaunchKernelGGL(mol_resonance_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2, out);
    return gi_launch_status();
}

extern "C" int gi_mol_kekulize(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                               const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                               const signed char* order2, int* status, signed char* edges_out, void* stream) {
    (void)hipGetLastError();
    if (Fe < 1 || Fe + 1 > GI_MAX_GROUPS) return Fe < 1 ? GI_EINVAL : GI_ELIMIT;
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe + 1)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if (G == 0) return 0;
    if (!nodes || !edges || !order2 || !status || !edges_out) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(Fe + 1) * N * 16;                                                  // <= 16 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_kekulize_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2,
                           status, edges_out);
    else
        hipLaunchKernelGGL(mol_kekulize_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, n_types, n_charges, n_imp_h, order2, status, edges_out);
    return gi_launch_status();
}
