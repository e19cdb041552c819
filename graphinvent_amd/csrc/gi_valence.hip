// Molecule validity on the device (gfx950): which of G generated molecules pass a valence test, and how many hydrogens
// each one takes — the part of the reference's `validity_tensor` (util.py:549-585, Analyzer.py:501-544: one
// `SanitizeMol` per molecule on the host) that is decidable from the labelled graph with the default bond set.  THIS IS A
// VALENCE TEST OF THE LABELLED GRAPH: no kekulisation, no aromaticity perception; the table of allowed valences is the
// caller's (analyze.ValenceRules), not RDKit's.
//
// mol_valence_kernel  one 256-lane WORKGROUP per molecule:
//   1, 2  gi_read_labelled of gi_molread.h, the front end it shares with gi_fingerprint.hip and gi_smiles.hip: all
//      waves read the molecule once (fp32 or int8) and check it while they read; in LDS one 128-bit adjacency row per
//      (bond type, node), and per node and segment (atom type, formal charge, implicit H) the number of set entries and
//      the lowest of them; n (given, or the leading rows with a set entry) and the bits of GI_MOL_MALFORMED (any of
//      them: nothing below is evaluated), GI_VAL_SELF_LOOP, GI_VAL_EMPTY;
//   3  one thread per atom: o2 = sum over bond types of order2[t] * popcount(row (t, i)), x = ceil(o2 / 2), v* = the lowest
//      allowed valence >= x of (atom type, charge), fill = v* - x; no v*: the atom is over its valence;
//   4  components by frontier expansion over the OR of the rows; at most N rounds whatever the data holds;
//   5  thread 0 writes the verdict and adds the molecule to the counters (integer atomics: any order, one result).
//      The counters live in a caller-owned scratch of GI_VAL_SCRATCH words that is zero between calls: the workgroup
//      that draws the last ticket moves them into `counts` and zeroes the scratch again, so no launch or memset is
//      needed to clear anything (calls that share a scratch must be ordered, e.g. by one stream).
// Integer arithmetic only.  Every index is bounded by the dims: i, j < N because they come from an offset < N N Fe, a
// segment index < its segment's size because it comes from an offset < Fn, a charge / type / H index is used only
// when the row is one-hot.  LDS: Fe N 16 B dynamic (<= 16 KB), ~8 KB static.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;

struct ValTables {
    const unsigned short* allowed;                           // [A * C]: bit v = total valence v is allowed
    const int* mass;                                         // [A] millidalton
    const i8* order2;                                        // [Fe] twice the bond order
    const i8* h_values;                                      // [H] the stored implicit-H counts (H > 0)
    int A, C, H, h_type, mass_h;
};

struct ValOut {
    float* valid;
    int* status;
    int* first_bad;
    i8* atom_valence;
    i8* atom_h;
    int* desc;
    int* counts;
    int* scratch;
};

template <typename T>
__global__ __launch_bounds__(NT) void mol_valence_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                         const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                         int Fe, ValTables tb, const void* __restrict__ term,
                                                         int term_dtype, int require_connected, ValOut out) {
    extern __shared__ unsigned adj[];                        // [Fe][N][4]: bit j of row (t, i): bond t between i and j
    __shared__ unsigned orr[MAXN][4];                        // the OR of a node's rows over the bond types
    __shared__ GiLabelled st;
    __shared__ unsigned vis[4], front[2][4];
    __shared__ int first_sh, sums[4];                        // sums: fills, atoms of type H, mass, bonds
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    if (tid < 4) { vis[tid] = 0u; front[0][tid] = 0u; front[1][tid] = 0u; sums[tid] = 0; }
    if (tid == 0) first_sh = 0x7fffffff;

    // ---- 1, 2: read and check; n and the well-formedness bits ---------------------------------------------
    GiLabelledNode me;
    const int n = gi_read_labelled<false>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes,
                                          nn_bytes, g, N, Fn, Fe, tb.A, tb.C, tb.H, tb.order2, tid, adj, st, orr, me);
    const bool sound = (st.flags & GI_MOL_MALFORMED) == 0;   // uniform
    const bool mine = sound && tid < n;                      // this thread owns atom `tid`

    // ---- 3: valences and the hydrogen fill -----------------------------------------------------------------
    int x = -1, h = -1, flags = 0;
    if (mine) {
        x = (gi_atom_order2(adj, tb.order2, N, Fe, tid) + 1) >> 1;
        const int a = st.seg_first[0][tid], c = st.seg_first[1][tid];     // a < A, c < C: the row is one-hot
        h = gi_hydrogen_fill((unsigned)tb.allowed[a * tb.C + c], x);
        if (h < 0) {
            flags |= GI_VAL_OVER;
            atomicMin(&first_sh, tid);
            h = 0;
        } else if (tb.H > 0 && (int)tb.h_values[st.seg_first[2][tid]] != h) {
            flags |= GI_VAL_H_MISMATCH;
        }
        if (me.arom) flags |= GI_VAL_AROMATIC;
        int above = 0;                                       // bonded partners of higher index
        for (int w = 0; w < 4; ++w) above += __popc(orr[tid][w] & ~gi_below_word(tid + 1, w));
        if (h) atomicAdd(&sums[0], h);
        if (a == tb.h_type) atomicAdd(&sums[1], 1);
        atomicAdd(&sums[2], tb.mass[a]);
        if (above) atomicAdd(&sums[3], above);
        x = min(x, 127);
    }

    // ---- 4: components ---------------------------------------------------------------------------------------
    int comps = 0;
    if (sound) {                                             // uniform
        int cur = 0;
        for (int round = 0; round < N; ++round) {
            __syncthreads();                                 // vis and front[cur] of the round before are complete
            bool all = true, empty = true;
            int seed = -1;
            for (int w = 3; w >= 0; --w) {
                const unsigned left = gi_below_word(n, w) & ~vis[w];
                if (left) { all = false; seed = 32 * w + __builtin_ctz(left); }
                if (front[cur][w]) empty = false;
            }
            if (all) break;
            if (empty) ++comps;                              // a new component starts at the lowest node not yet seen
            const bool in_front = empty ? tid == seed : (tid < n && ((front[cur][tid >> 5] >> (tid & 31)) & 1u));
            __syncthreads();                                 // everybody has read vis and front[cur]
            if (tid < 4) front[cur ^ 1][tid] = 0u;
            if (empty && tid == seed) atomicOr(&vis[tid >> 5], 1u << (tid & 31));
            __syncthreads();
            unsigned reach[4] = {0u, 0u, 0u, 0u};
            if (in_front)
                for (int w = 0; w < 4; ++w) reach[w] = orr[tid][w] & gi_below_word(n, w) & ~vis[w];
            __syncthreads();                                 // vis is read before anybody adds to it
            if (in_front)
                for (int w = 0; w < 4; ++w)
                    if (reach[w]) { atomicOr(&front[cur ^ 1][w], reach[w]); atomicOr(&vis[w], reach[w]); }
            cur ^= 1;
        }
        if (comps > 1) flags |= GI_VAL_FRAGMENTS;
    }
    if (flags) atomicOr(&st.flags, flags);
    __syncthreads();

    // ---- 5: outputs ------------------------------------------------------------------------------------------
    for (int a = tid; a < N; a += NT) {                      // N <= 128 < NT: thread a is atom a's owner
        out.atom_valence[(size_t)g * N + a] = (i8)x;
        out.atom_h[(size_t)g * N + a] = (i8)h;
    }
    if (tid == 0) {
        const int status = st.flags;
        int invalid = GI_MOL_MALFORMED | GI_VAL_EMPTY | GI_VAL_SELF_LOOP | GI_VAL_OVER;
        if (require_connected) invalid |= GI_VAL_FRAGMENTS;
        const int valid = (status & invalid) == 0;
        out.status[g] = status;
        out.valid[g] = valid ? 1.f : 0.f;
        out.first_bad[g] = first_sh == 0x7fffffff ? -1 : first_sh;
        int* d = out.desc + (size_t)g * GI_VAL_DESC;
        const int bonds = sums[3];
        d[0] = sound ? n : 0;
        d[1] = sums[0] + sums[1];
        d[2] = sums[2] + sums[0] * tb.mass_h;
        d[3] = bonds;
        d[4] = comps;
        d[5] = sound ? bonds - n + comps : 0;
        int terminated = 0;
        if (term) terminated = term_dtype == GI_DTYPE_I8 ? ((const i8*)term)[g] != 0 : ((const float*)term)[g] != 0.f;
        int* sc = out.scratch;
        if (valid) atomicAdd(&sc[0], 1);
        if (terminated) atomicAdd(&sc[1], 1);
        if (valid && terminated) atomicAdd(&sc[2], 1);
        __threadfence();                                     // the sums before the ticket
        if (atomicAdd(&sc[3], 1) == (int)gridDim.x - 1) {    // the last workgroup: every sum is complete
            __threadfence();
            for (int k = 0; k < 3; ++k) out.counts[k] = atomicExch(&sc[k], 0);
            out.counts[3] = (int)gridDim.x;
            atomicExch(&sc[3], 0);                           // the scratch is zero again for the next call
        }
    }
}

}  // namespace

extern "C" int gi_mol_valence(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                              const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                              const unsigned short* allowed, const int* mass, const signed char* order2,
                              const signed char* h_values, int h_type, int mass_h, const void* termination,
                              int term_dtype, int require_connected, float* valid, int* status, int* first_bad,
                              signed char* atom_valence, signed char* atom_h, int* desc, int* counts, int* scratch,
                              void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (term_dtype != GI_DTYPE_F32 && term_dtype != GI_DTYPE_I8) return GI_EINVAL;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if (h_type < -1 || h_type >= n_types) return GI_EINVAL;
    if (G == 0) return 0;
    if (!nodes || !edges || !allowed || !mass || !order2 || (n_imp_h > 0 && !h_values) || !valid || !status ||
        !first_bad || !atom_valence || !atom_h || !desc || !counts || !scratch)
        return GI_EINVAL;
    const ValTables tb = {allowed, mass, order2, h_values, n_types, n_charges, n_imp_h, h_type, mass_h};
    const ValOut out = {valid, status, first_bad, atom_valence, atom_h, desc, counts, scratch};
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned);                                      // <= 16 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_valence_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, tb, termination, term_dtype,
                           require_connected, out);
    else
        hipLaunchKernelGGL(mol_valence_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, tb, termination, term_dtype, require_connected, out);
    return gi_launch_status();
}
