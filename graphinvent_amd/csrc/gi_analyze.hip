// Read-out of generated molecules on the device (gfx950): the tensor bookkeeping of `Analyzer.get_molecular_properties`
// (Analyzer.py:311-599) and of `graph_to_graph` (GraphGenerator.py:659-804, GraphGeneratorRL.py:725-) over
// nodes [G, N, Fn] / edges [G, N, N, Fe] (fp32 or int8) and n_nodes [G], which the reference walks molecule by molecule,
// node by node and bond by bond from Python with one device-to-host synchronisation per step.
//
// mol_props_kernel   workgroups stride over the graphs.  Per graph every byte is read once (gi_for_each_nonzero of
//                    gi_molread.h, the reader of all the molecule kernels); the VALUE of a non-zero entry goes to LDS:
//                    the column sums of the node rows, the per-node degree (all N columns, all bond types), the sum per
//                    bond type, the non-zero-row mask.  Then the graph's n_nodes and its nodes' degrees are binned.  The
//                    bins are int32 in LDS, flushed with one 64-bit atomicAdd per non-zero bin at the end (and every
//                    `flush_every` graphs, so that they cannot wrap).  Integer sums do not depend on the order, so the
//                    result is deterministic.  The workgroup that finishes last turns the totals into the reference's
//                    fp32 values: the exact integer as fp32, then one correctly rounded fp32 division.
// mol_decode_kernel  one workgroup per graph.  The atom records: one thread per (node, segment) scans the segment.  The
//                    bond records: the triples (i, j, type), i < j, of the non-zero entries in the order of the flat
//                    [N, N, Fe] index, i.e. `torch.nonzero(edge_features * triu_mask)`'s: chunks of 256 granules, a
//                    thread's kept entries as a bit mask, their ranks from a wave scan of the popcounts plus the waves'
//                    totals in LDS (the order-preserving compaction of gi_eval.hip with several entries per thread).
// Every loop is bounded by the dims whatever the data holds, every index is checked against its buffer.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int NW = NT / 64;
constexpr int MAXN = GI_MAX_NODES;
constexpr int MAXF = GI_ANALYZE_MAX_FN;
constexpr int EB = GI_ANALYZE_EDGE_BINS;

// layout of the totals (u64) and of the fp32 results: [n_nodes_hist | node columns | n_edges_hist | edge features], then
// totals: termination sum, finished workgroups; results: avg_n_nodes, avg_n_edges, fraction_properly_terminated
template <typename T>
__global__ __launch_bounds__(NT) void mol_props_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                       const void* __restrict__ n_nodes, int nn_bytes,
                                                       const void* __restrict__ term, int term_dtype, int G, int N,
                                                       int Fn, int Fe, int max_n, int flush_every, u64* totals,
                                                       float* __restrict__ out) {
    __shared__ int bins[MAXN + 1 + MAXF + EB + GI_MAX_GROUPS + 1];
    __shared__ int deg[MAXN];
    __shared__ unsigned present[4];
    __shared__ int last_sh;
    const int tid = threadIdx.x;
    const int H = max_n + 1;                                   // length of n_nodes_hist in the totals
    int* hn = bins;                                            // [N + 1]: a count above N is not binned
    int* col = hn + MAXN + 1;
    int* eh = col + MAXF;
    int* ef = eh + EB;
    int* ts = ef + GI_MAX_GROUPS;
    const int nb_lds = MAXN + 1 + MAXF + EB + GI_MAX_GROUPS + 1;
    const int len_n = N * Fn, len_e = N * N * Fe;
    auto flush = [&]() {                                       // between two barriers of the caller
        for (int b = tid; b < nb_lds; b += NT) {
            const int v = bins[b];
            if (v == 0) continue;
            int dst;
            if (b <= MAXN) dst = b;                            // only bins <= min(N, max_n) are ever non-zero
            else if (b < MAXN + 1 + MAXF) dst = H + (b - MAXN - 1);
            else if (b < MAXN + 1 + MAXF + EB) dst = H + Fn + (b - MAXN - 1 - MAXF);
            else if (b < nb_lds - 1) dst = H + Fn + EB + (b - MAXN - 1 - MAXF - EB);
            else dst = H + Fn + EB + Fe;
            atomicAdd(&totals[dst], (u64)(long long)v);
            bins[b] = 0;
        }
    };
    for (int b = tid; b < nb_lds; b += NT) bins[b] = 0;
    int since = 0;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {          // uniform over the workgroup
        for (int i = tid; i < MAXN; i += NT) deg[i] = 0;
        if (tid < 4) present[tid] = 0u;
        __syncthreads();
        gi_for_each_nonzero(nodes + (size_t)g * len_n, len_n, tid, [&](int o, T x) {
            const int i = o / Fn;
            atomicAdd(&col[o - i * Fn], (int)x);
            atomicOr(&present[i >> 5], 1u << (i & 31));
        });
        gi_for_each_nonzero(edges + (size_t)g * len_e, len_e, tid, [&](int o, T x) {
            const int e = o / Fe, i = e / N, v = (int)x;
            atomicAdd(&deg[i], v);
            atomicAdd(&ef[o - e * Fe], v);
        });
        __syncthreads();
        const int n = n_nodes ? (int)gi_load_count(n_nodes, nn_bytes, g)   // narrowed: a count past int wraps
                              : __popc(present[0]) + __popc(present[1]) + __popc(present[2]) + __popc(present[3]);
        if (tid == 0) {
            if (n >= 0 && n <= N && n <= max_n) hn[n] += 1;
            if (term) ts[0] += term_dtype == GI_DTYPE_I8 ? (int)((const i8*)term)[g] : (int)((const float*)term)[g];
        }
        if (tid < min(n, N)) {                                 // hist[degree - 1] with Python's index: 0 -> the last bin
            const int d = min(deg[tid], EB);
            const int idx = d >= 1 ? d - 1 : d + EB - 1;
            if (idx >= 0) atomicAdd(&eh[idx], 1);
        }
        __syncthreads();
        if (++since == flush_every) {
            flush();
            since = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    flush();
    // ---- the workgroup that finishes last forms the results -------------------------------------------------
    __threadfence();
    __syncthreads();
    const int nb = H + Fn + EB + Fe;                            // bins of the totals; [nb] termination, [nb + 1] done
    if (tid == 0) {
        const u64 prev = atomicAdd(&totals[nb + 1], 1ull);
        last_sh = prev == (u64)gridDim.x - 1;
    }
    __syncthreads();
    if (!last_sh) return;
    __threadfence();
    auto total = [&](int b) {
        return (long long)__hip_atomic_load(&totals[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int b = tid; b < nb; b += NT) {
        const float x = (float)total(b);
        out[b] = b >= H + Fn + EB ? x / 2.f : x;               // edge_feature_hist: the plane's sum / 2
    }
    if (tid == 0) {
        long long sn = 0, se = 0, ce = 0;
        for (int k = 0; k < H; ++k) sn += (long long)k * total(k);
        for (int k = 0; k < EB; ++k) {
            const long long c = total(H + Fn + k);
            se += (long long)(k + 1) * c;
            ce += c;
        }
        out[nb] = (float)sn / (float)G;
        out[nb + 1] = (float)se / (float)ce;                    // 0 / 0 = NaN without a node, as the reference
        out[nb + 2] = (float)total(nb) / (float)G;
    }
}

struct Segs {
    int n, size[4];
};

template <typename T>
__global__ __launch_bounds__(NT) void mol_decode_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                        const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                        int Fe, Segs segs, int max_bonds, i8* __restrict__ atoms,
                                                        short* __restrict__ bonds, int* __restrict__ n_bonds,
                                                        int* __restrict__ status) {
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ int wtot[NW];
    __shared__ int err_sh;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int len_n = N * Fn, len_e = N * N * Fe, S = segs.n;
    const T* nd = nodes + (size_t)g * len_n;
    const T* ed = edges + (size_t)g * len_e;
    const int n = min(max((int)gi_load_count(n_nodes, nn_bytes, g), 0), N);
    if (tid == 0) err_sh = 0;
    int err = 0;

    // ---- atoms: the index of the set entry inside each segment ---------------------------------------------
    for (int idx = tid; idx < N * S; idx += NT) {
        const int i = idx / S, s = idx - i * S;
        int off = 0;
        for (int k = 0; k < s; ++k) off += segs.size[k];
        const T* row = nd + i * Fn + off;
        int first = -1, count = 0;
        for (int f = 0; f < segs.size[s]; ++f) {
            const T x = row[f];
            if (x == (T)0) continue;
            if (!gi_is01(x)) err |= GI_MOL_VALUE;
            if (first < 0) first = f;
            ++count;
        }
        if (i < n && count != 1) err |= GI_MOL_ONEHOT;
        atoms[((size_t)g * N + i) * S + s] = (i8)(i < n ? first : -1);
    }

    // ---- bonds: ordered compaction of the upper triangle's non-zero entries ---------------------------------
    const int P = gi_granule_count(ed, len_e);
    short* out = bonds + (size_t)g * max_bonds * 3;
    int base = 0;                                               // bonds of the previous chunks
    for (int c0 = 0; c0 < P; c0 += NT) {                        // uniform
        const int q = c0 + tid;
        T v[E];
        int o0 = 0, c = 0;
        bool any = false;
        if (q < P) {
            c = gi_load_granule(ed, len_e, q, o0, v);
#pragma unroll
            for (int k = 0; k < E; ++k) any |= v[k] != (T)0;
        }
        unsigned mask = 0;
        if (any) {
            const int e = o0 / Fe;
            int t = o0 - e * Fe, i = e / N, j = e - i * N;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                if (k < c && v[k] != (T)0) {
                    if (!gi_is01(v[k])) err |= GI_MOL_VALUE;
                    if (i < j) {
                        mask |= 1u << k;
                        if (j >= n) err |= GI_MOL_BOND_PAST_N;
                        for (int t2 = 0; t2 < t; ++t2)          // an earlier type of the same pair
                            if (ed[o0 + k - t + t2] != (T)0) err |= GI_MOL_MULTI_BOND;
                    }
                }
                if (++t == Fe) {
                    t = 0;
                    if (++j == N) { j = 0; ++i; }
                }
            }
        }
        const int cnt = __popc(mask);
        int inc = cnt;                                          // inclusive scan over the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int y = __shfl_up(inc, s);
            if (lane >= s) inc += y;
        }
        __syncthreads();                                        // the previous chunk's wtot reads are done
        if (lane == 63) wtot[wid] = inc;
        __syncthreads();
        int off = base + inc - cnt;
        for (int w = 0; w < wid; ++w) off += wtot[w];
        for (int w = 0; w < NW; ++w) base += wtot[w];
        if (mask) {
            const int e = o0 / Fe;
            int t = o0 - e * Fe, i = e / N, j = e - i * N;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                if ((mask >> k) & 1u) {
                    if (off < max_bonds) {
                        out[off * 3 + 0] = (short)i;
                        out[off * 3 + 1] = (short)j;
                        out[off * 3 + 2] = (short)t;
                    }
                    ++off;
                }
                if (++t == Fe) {
                    t = 0;
                    if (++j == N) { j = 0; ++i; }
                }
            }
        }
    }
    if (base > max_bonds) err |= GI_MOL_OVERFLOW;
    for (int k = min(base, max_bonds) * 3 + tid; k < max_bonds * 3; k += NT) out[k] = (short)-1;
    if (err) atomicOr(&err_sh, err);                            // err_sh was zeroed before the loop's barriers (P >= 1)
    __syncthreads();
    if (tid == 0) {
        n_bonds[g] = base;
        status[g] = err_sh;
    }
}

// any EINVAL comes before the Fn limit
int check_args(int G, int N, int Fn, int Fe, int dtype, int nn_bytes) {
    if (const int rc = gi_mol_check_types(dtype, nn_bytes)) return rc;
    return gi_mol_check_dims(G, N, Fn, Fe);
}

}  // namespace

extern "C" int gi_mol_properties(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                                 const void* n_nodes, int n_nodes_bytes, const void* termination, int term_dtype,
                                 int max_n_nodes, unsigned long long* totals, float* out, void* stream) {
    (void)hipGetLastError();
    if (const int rc = check_args(G, N, Fn, Fe, dtype, n_nodes_bytes)) return rc;
    if (max_n_nodes < 0 || max_n_nodes > GI_ANALYZE_MAX_HIST) return GI_EINVAL;
    if (termination && term_dtype != GI_DTYPE_F32 && term_dtype != GI_DTYPE_I8) return GI_EINVAL;
    if (G == 0) return 0;
    if (!nodes || !edges || !totals || !out) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const int grid = G < 1024 ? G : 1024;
    const int flush_every = (1 << 30) / (N * N * 128) > 0 ? (1 << 30) / (N * N * 128) : 1;   // |entry| <= 128
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_props_kernel<float>, dim3(grid), dim3(NT), 0, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, termination, term_dtype, G, N, Fn, Fe,
                           max_n_nodes, flush_every, totals, out);
    else
        hipLaunchKernelGGL(mol_props_kernel<i8>, dim3(grid), dim3(NT), 0, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, termination, term_dtype, G, N, Fn, Fe, max_n_nodes, flush_every,
                           totals, out);
    return gi_launch_status();
}

extern "C" int gi_mol_decode(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                             const void* n_nodes, int n_nodes_bytes, int n_seg, const int* seg, int max_bonds,
                             signed char* atoms, short* bonds, int* n_bonds, int* status, void* stream) {
    (void)hipGetLastError();
    if (const int rc = check_args(G, N, Fn, Fe, dtype, n_nodes_bytes)) return rc;
    if (n_seg < 2 || n_seg > 4 || !seg || max_bonds < 1 || max_bonds > (1 << 20)) return GI_EINVAL;
    Segs segs;
    segs.n = n_seg;
    int sum = 0;
    for (int k = 0; k < 4; ++k) {
        segs.size[k] = k < n_seg ? seg[k] : 0;
        if (segs.size[k] < (k < n_seg ? 1 : 0) || segs.size[k] > 127) return GI_EINVAL;   // an index fits int8
        sum += segs.size[k];
    }
    if (sum != Fn) return GI_EINVAL;
    if (G == 0) return 0;
    if (!nodes || !edges || !n_nodes || !atoms || !bonds || !n_bonds || !status) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_decode_kernel<float>, dim3(G), dim3(NT), 0, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, segs, max_bonds, atoms, bonds,
                           n_bonds, status);
    else
        hipLaunchKernelGGL(mol_decode_kernel<i8>, dim3(G), dim3(NT), 0, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, segs, max_bonds, atoms, bonds, n_bonds, status);
    return gi_launch_status();
}
