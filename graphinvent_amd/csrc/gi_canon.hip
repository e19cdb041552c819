// Molecule identity on the device (gfx950): which of G generated molecules are the same labelled graph, which the
// reference decides on the host from canonical SMILES (util.py:549-585 `current_smiles in smiles`, Analyzer.py:480-499,
// Workflow.py:862-898).  Here: a canonical node order by colour refinement with individualisation (no backtracking),
// the canonical molecule nodes[order], edges[order][:, order], a 128-bit key of it, first occurrences inside a call by
// key + byte comparison, and a key-only table across calls.
//
// mol_canon_kernel   one 256-lane WORKGROUP per molecule (not one wave: a molecule is up to 128 x 128 x 8 entries, and
//                    reading it is what takes the time; the refinement rounds are short and use the workgroup barrier,
//                    the same code for every n).
//   1  all waves read the molecule once (gi_for_each_nonzero of gi_molread.h; fp32 or int8), check it
//      (gi_mol_structure, shared with gi_valence.hip) and build in LDS one 128-bit adjacency row per (bond type,
//      node) and one bit row per node's feature row (feature f at bit 31 - f % 32 of word f / 32, so that comparing the words as unsigned
//      numbers compares the rows as byte strings);
//   2  initial colour = the rank of the feature row among the molecule's n rows; one thread per node;
//   3  rounds: h_i = sum over (t, j) with bond t between i and j of mix64(t << 32 | col_j) (commutative, so the order
//      is irrelevant), col'_i = #{j : (col_j, h_j) < (col_i, h_i)}.  The old colour leads the key, so cells only split.
//      A round that did not raise the number of cells ends a refinement; the same round then individualises: in the
//      non-singleton cell of smallest colour r the member of lowest input index keeps r, the others get r + 1 (free,
//      because a cell of size s owns the ranks r .. r + s - 1);
//   4  order = nodes by ascending colour; the key: two independent 64-bit sums of per-set-entry terms of the canonical
//      molecule with n mixed in; the canonical molecule is stored in 16-byte pieces between its ragged ends
//      (store_bytes of gi_molread.h).
// LDS: Fe N 16 B of adjacency (<= 16 KB) + N ceil(Fn / 32) 4 B of feature bits (<= 8 KB) dynamic, ~3 KB static.
// Every loop is bounded by the dims whatever the data holds: every round raises the cell count or individualises, both
// at most n - 1 times, and the loop is cut at 2 N + 2 rounds regardless; colours stay below n, every index below N.
// A molecule that fails a check gets the identity order over all N slots, a zero canonical molecule, its GI_MOL_* bits
// and a key made of its index; gi_mol_unique / gi_mol_seen_add never compare such a molecule with anything.
//
// mol_unique_insert_kernel  one wave per molecule: the scheme of route_insert_kernel (gi_route.hip) — probe an
//                    open-addressing table from the key, claim an empty slot or join the slot whose owner has the same
//                    key AND the same canonical bytes, atomicMin of the molecule index into the slot.  Which molecule
//                    owns a slot depends on timing, nothing visible does.
// mol_seen_kernel    one thread per molecule, a caller-owned table of 128-bit keys (two non-zero words, zero = empty):
//                    compare-and-swap the first word into an empty slot (or find it there), then the second word into
//                    ITS empty cell: whoever sets the second word has inserted the key, whoever finds its own second
//                    word has found it, anybody else walks on.  No thread ever waits for another; a probe ends after
//                    `capacity` slots.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr unsigned EMPTY = 0xFFFFFFFFu;
constexpr int NO_TARGET = 0x7fffffff;

__device__ __forceinline__ u64 tagged(int tag, u64 x) { return mix64(((u64)tag << 40) | x); }
__device__ __forceinline__ u64 nonzero_word(u64 x) { return x ? x : 1ull; }

template <typename T>
__global__ __launch_bounds__(NT) void mol_canon_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                       const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                       int Fe, int* __restrict__ order_out, int* __restrict__ rank_out,
                                                       u64* __restrict__ key_out, int* __restrict__ status_out,
                                                       i8* __restrict__ out_nodes, i8* __restrict__ out_edges) {
    extern __shared__ unsigned smem[];
    const int W = (Fn + 31) >> 5;                            // words of a node's feature bits
    unsigned* adj = smem;                                    // [Fe][N][4]: bit j of row (t, i): bond t between i and j
    unsigned* nbits = smem + Fe * N * 4;                     // [N][W]
    __shared__ u64 hs[MAXN];
    __shared__ u64 ksum[2];
    __shared__ int col[MAXN], order[MAXN];
    __shared__ unsigned present[4];
    __shared__ int err_sh, tgt_sh;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int len_n = N * Fn, len_e = N * N * Fe;
    const T* nd = nodes + (size_t)g * len_n;
    const T* ed = edges + (size_t)g * len_e;
    for (int i = tid; i < Fe * N * 4 + N * W; i += NT) smem[i] = 0u;
    if (tid < MAXN) order[tid] = tid;
    if (tid < 4) present[tid] = 0u;
    if (tid < 2) ksum[tid] = 0ull;
    if (tid == 0) { err_sh = 0; tgt_sh = NO_TARGET; }
    __syncthreads();

    // ---- 1: read and check -------------------------------------------------------------------------------
    int err = 0;
    gi_for_each_nonzero(nd, len_n, tid, [&](int o, T x) {
        if (!gi_is01(x)) err |= GI_MOL_VALUE;
        const int i = o / Fn, f = o - i * Fn;
        atomicOr(&nbits[i * W + (f >> 5)], 1u << (31 - (f & 31)));
        atomicOr(&present[i >> 5], 1u << (i & 31));
    });
    gi_for_each_nonzero(ed, len_e, tid, [&](int o, T x) {
        if (!gi_is01(x)) err |= GI_MOL_VALUE;
        const int e = o / Fe, t = o - e * Fe, i = e / N, j = e - i * N;
        atomicOr(&adj[(t * N + i) * 4 + (j >> 5)], 1u << (j & 31));
    });
    __syncthreads();
    const int n = gi_mol_structure(adj, present, n_nodes, nn_bytes, g, N, Fe, tid, err);
    if (err) atomicOr(&err_sh, err);
    __syncthreads();
    const int status = err_sh;                               // uniform; not written again
    const bool sound = status == 0;
    const bool mine = sound && tid < n;                      // this thread owns node `tid`

    // ---- 2: initial colours: the rank of the feature row ----------------------------------------------------
    int cells = n;
    {
        int r = 0;
        bool first = true;
        if (mine) {
            for (int j = 0; j < n; ++j) {
                int cmp = 0;                                 // row_j <=> row_i
                for (int w = 0; w < W && cmp == 0; ++w) {
                    const unsigned a = nbits[j * W + w], b = nbits[tid * W + w];
                    cmp = a < b ? -1 : a > b ? 1 : 0;
                }
                r += cmp < 0;
                if (cmp == 0 && j < tid) first = false;
            }
            col[tid] = r;
        }
        cells = __syncthreads_count(mine && first);
    }

    // ---- 3: refine, individualise ------------------------------------------------------------------------
    if (sound) {                                             // uniform
        for (int it = 0; it < 2 * N + 2 && cells < n; ++it) {
            int c = 0, r = 0;
            u64 h = 0;
            bool first = true, dup = false;
            if (mine) {
                c = col[tid];
                for (int t = 0; t < Fe; ++t)
                    for (int w = 0; w < 4; ++w) {
                        unsigned bits = adj[(t * N + tid) * 4 + w];
                        while (bits) {
                            const int j = 32 * w + __builtin_ctz(bits);
                            bits &= bits - 1;
                            h += mix64(((u64)t << 32) | (u64)col[j]);
                        }
                    }
                hs[tid] = h;
            }
            __syncthreads();
            if (mine)
                for (int j = 0; j < n; ++j) {
                    const int cj = col[j];
                    const u64 hj = hs[j];
                    r += cj < c || (cj == c && hj < h);
                    const bool eq = cj == c && hj == h;
                    first = first && !(eq && j < tid);
                    dup = dup || (eq && j != tid);
                }
            const int c2 = __syncthreads_count(mine && first);
            if (c2 == cells) {                               // nothing split (so r == c): individualise
                if (mine && dup) atomicMin(&tgt_sh, (r << 7) | tid);
                __syncthreads();
                const int tg = tgt_sh;
                if (mine) col[tid] = (tg != NO_TARGET && r == (tg >> 7) && tid != (tg & 127)) ? r + 1 : r;
                cells = c2 + 1;
                __syncthreads();
                if (tid == 0) tgt_sh = NO_TARGET;            // read again two barriers from here at the earliest
            } else {
                if (mine) col[tid] = r;
                cells = c2;
                __syncthreads();
            }
        }
        if (mine) order[col[tid]] = tid;                     // colours are < n and, the loop having ended, distinct
    }
    __syncthreads();

    // ---- 4: outputs ------------------------------------------------------------------------------------------
    const int n_out = sound ? n : N;
    if (tid == 0) status_out[g] = status;
    for (int a = tid; a < N; a += NT) {
        order_out[(size_t)g * N + a] = a < n_out ? order[a] : -1;
        rank_out[(size_t)g * N + a] = a < n_out ? (sound ? col[a] : a) : -1;
    }
    if (sound) {
        u64 k0 = 0, k1 = 0;
        for (int idx = tid; idx < n * W; idx += NT) {
            const int a = idx / W, w = idx - a * W;
            unsigned bits = nbits[order[a] * W + w];
            while (bits) {
                const int f = 32 * w + 31 - __builtin_ctz(bits);
                bits &= bits - 1;
                const u64 x = (u64)(a * Fn + f);
                k0 += tagged(1, x);
                k1 += tagged(4, x);
            }
        }
        for (int idx = tid; idx < Fe * n; idx += NT) {
            const int t = idx / n, a = idx - t * n;
            for (int w = 0; w < 4; ++w) {
                unsigned bits = adj[(t * N + order[a]) * 4 + w];
                while (bits) {
                    const int j = 32 * w + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const u64 y = (u64)((a * N + col[j]) * Fe + t);
                    k0 += tagged(2, y);
                    k1 += tagged(5, y);
                }
            }
        }
        k0 = wave_sum64(k0);
        k1 = wave_sum64(k1);
        if (lane == 0) { atomicAdd(&ksum[0], k0); atomicAdd(&ksum[1], k1); }
        __syncthreads();
        if (tid == 0) {
            key_out[2 * (size_t)g] = nonzero_word(ksum[0] + mix64((u64)n));
            key_out[2 * (size_t)g + 1] = nonzero_word(ksum[1] + tagged(3, (u64)n));
        }
    } else if (tid == 0) {
        key_out[2 * (size_t)g] = nonzero_word(tagged(6, (u64)g));
        key_out[2 * (size_t)g + 1] = nonzero_word(tagged(7, (u64)g));
    }
    if (out_nodes)
        store_bytes(out_nodes + (size_t)g * len_n, len_n, tid, N, 1, Fn,
                    [&](int a, int) { return sound && a < n ? order[a] : -1; },
                    [&](int s, int f) { return (int)((nbits[s * W + (f >> 5)] >> (31 - (f & 31))) & 1u); });
    if (out_edges)
        store_bytes(out_edges + (size_t)g * len_e, len_e, tid, N, N, Fe,
                    [&](int a, int b) { return sound && a < n && b < n ? (order[a] << 7) | order[b] : -1; },
                    [&](int s, int t) {
                        const int i = s >> 7, j = s & 127;
                        return (int)((adj[(t * N + i) * 4 + (j >> 5)] >> (j & 31)) & 1u);
                    });
}

// bytes a[0, len) == b[0, len), the wave's lanes striding over them; words where both addresses allow
__device__ __forceinline__ bool wave_differs(const i8* a, const i8* b, int len, int lane) {
    bool diff = false;
    if ((((uintptr_t)a | (uintptr_t)b) & 3) == 0) {
        const int words = len >> 2;
        const unsigned* wa = (const unsigned*)a;
        const unsigned* wb = (const unsigned*)b;
        for (int q = lane; q < words; q += 64) diff |= wa[q] != wb[q];
        for (int q = (words << 2) + lane; q < len; q += 64) diff |= a[q] != b[q];
    } else {
        for (int q = lane; q < len; q += 64) diff |= a[q] != b[q];
    }
    return diff;
}

__global__ __launch_bounds__(256) void mol_unique_insert_kernel(const u64* __restrict__ key, const i8* __restrict__ cn,
                                                                int pitch_n, const i8* __restrict__ ce, int pitch_e,
                                                                const int* __restrict__ status,
                                                                const i8* __restrict__ mask, int G,
                                                                unsigned* __restrict__ slot,
                                                                unsigned* __restrict__ minidx, unsigned tmask,
                                                                int* __restrict__ slot_of) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= G) return;
    if (mask && mask[r] == 0) { if (lane == 0) slot_of[r] = -1; return; }       // not in the call at all
    if (status[r] != 0) { if (lane == 0) slot_of[r] = -2; return; }             // a class of its own
    const u64 k0 = key[2 * (size_t)r], k1 = key[2 * (size_t)r + 1];
    unsigned s = (unsigned)k0 & tmask;
    for (unsigned it = 0; it <= tmask; ++it, s = (s + 1) & tmask) {
        unsigned v = 0;
        if (lane == 0) v = atomicCAS(&slot[s], EMPTY, (unsigned)r);
        v = (unsigned)__shfl((int)v, 0);
        if (v == EMPTY || v == (unsigned)r) break;
        if (v >= (unsigned)G) continue;                       // cannot happen: only indices < G are inserted
        if (key[2 * (size_t)v] != k0 || key[2 * (size_t)v + 1] != k1) continue;
        bool diff = wave_differs(cn + (size_t)r * pitch_n, cn + (size_t)v * pitch_n, pitch_n, lane);
        diff |= wave_differs(ce + (size_t)r * pitch_e, ce + (size_t)v * pitch_e, pitch_e, lane);
        if (!__any(diff)) break;
    }
    // the table has more slots than molecules, so the walk ended on a claimed or a joined slot
    if (lane == 0) { slot_of[r] = (int)s; atomicMin(&minidx[s], (unsigned)r); }
}

__global__ __launch_bounds__(256) void mol_unique_finish_kernel(const int* __restrict__ slot_of,
                                                                const unsigned* __restrict__ minidx,
                                                                const int* __restrict__ status, int G,
                                                                int* __restrict__ rep, float* __restrict__ unique,
                                                                int* __restrict__ counts) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    int bits = 0, in = 0, cls = 0;
    if (r < G) {
        bits = status[r];
        const int s = slot_of[r];
        const int p = s == -1 ? -1 : s == -2 ? r : (int)minidx[s];
        rep[r] = p;
        unique[r] = (p >= 0 && p != r) ? 0.f : 1.f;
        in = p >= 0;
        cls = p == r;
    }
    // integer sums: any order gives the same result
    const int in_w = __popcll(__ballot(in)), cls_w = __popcll(__ballot(cls));
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) bits |= __shfl_xor(bits, s);
    if ((threadIdx.x & 63) == 0) {
        if (bits) atomicOr(&counts[0], bits);
        if (in_w) atomicAdd(&counts[1], in_w);
        if (cls_w) atomicAdd(&counts[2], cls_w);
    }
}

__global__ __launch_bounds__(256) void mol_seen_kernel(const u64* __restrict__ key, const int* __restrict__ status,
                                                       const int* __restrict__ rep, int G, u64* __restrict__ table,
                                                       u64 cmask, int* __restrict__ info, int* __restrict__ is_new) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= G) return;
    if (rep[r] != r) { is_new[r] = 0; return; }              // masked out, or a later copy inside this call
    if (status[r] != 0) { is_new[r] = 1; return; }           // never equal to anything, never stored
    const u64 k0 = key[2 * (size_t)r], k1 = key[2 * (size_t)r + 1];      // both non-zero
    u64 s = k0 & cmask;
    int fresh = 1;
    bool placed = false;
    for (u64 it = 0; it <= cmask; ++it, s = (s + 1) & cmask) {
        const u64 a = atomicCAS(&table[2 * s], 0ull, k0);
        if (a != 0ull && a != k0) continue;
        const u64 b = atomicCAS(&table[2 * s + 1], 0ull, k1);
        if (b == 0ull) { atomicAdd(&info[0], 1); placed = true; break; }         // this thread inserted the key
        if (b == k1) { fresh = 0; placed = true; break; }                        // it is there already
    }
    if (!placed) atomicOr(&info[1], GI_SEEN_FULL);           // every slot holds another key
    is_new[r] = fresh;
}

struct UniqueWs { size_t slot, minidx, slot_of, total; unsigned tsize; };

__host__ size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }

UniqueWs unique_layout(int G) {
    UniqueWs w;
    unsigned T = 64;
    while ((size_t)T < 2 * (size_t)G) T <<= 1;
    w.tsize = T;
    size_t o = 0;
    w.slot = o; o += r16((size_t)T * 4);
    w.minidx = o; o += r16((size_t)T * 4);                   // directly behind slot: one memset sets both
    w.slot_of = o; o += r16((size_t)G * 4);
    w.total = o;
    return w;
}

constexpr int MAX_UNIQUE = 1 << 29;                          // 2 G must fit the 32-bit table index

}  // namespace

extern "C" int gi_mol_canon(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                            const void* n_nodes, int n_nodes_bytes, int* order, int* rank, unsigned long long* key,
                            int* status, signed char* out_nodes, signed char* out_edges, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (G == 0) return 0;
    if (!nodes || !edges || !order || !rank || !key || !status) return GI_EINVAL;
    if ((const void*)out_nodes == nodes || (const void*)out_edges == edges) return GI_EINVAL;      // not in place
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)Fe * N * 4 + (size_t)N * ((Fn + 31) / 32)) * sizeof(unsigned);     // <= 24 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_canon_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, order, rank, (u64*)key, status,
                           out_nodes, out_edges);
    else
        hipLaunchKernelGGL(mol_canon_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, order, rank, (u64*)key, status, out_nodes, out_edges);
    return gi_launch_status();
}

extern "C" long long gi_mol_unique_ws_bytes(int G) {
    if (G < 0) return GI_EINVAL;
    if (G > MAX_UNIQUE) return GI_ELIMIT;
    return (long long)unique_layout(G).total;
}

extern "C" int gi_mol_unique(int G, int N, int Fn, int Fe, const unsigned long long* key,
                             const signed char* canon_nodes, const signed char* canon_edges, const int* status,
                             const signed char* mask, void* ws, int* rep, float* unique, int* counts, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (G > MAX_UNIQUE) return GI_ELIMIT;
    if (!counts) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, GI_MOL_COUNTS * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (G == 0) return 0;
    if (!key || !canon_nodes || !canon_edges || !status || !ws || !rep || !unique) return GI_EINVAL;
    const UniqueWs w = unique_layout(G);
    char* base = (char*)ws;
    unsigned* slot = (unsigned*)(base + w.slot);
    unsigned* minidx = (unsigned*)(base + w.minidx);
    int* slot_of = (int*)(base + w.slot_of);
    e = hipMemsetAsync(slot, 0xFF, w.slot_of - w.slot, st);                       // slot and minidx
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mol_unique_insert_kernel, dim3(gi_cdiv(G, 4)), dim3(256), 0, st, (const u64*)key, canon_nodes,
                       N * Fn, canon_edges, N * N * Fe, status, mask, G, slot, minidx, w.tsize - 1, slot_of);
    hipLaunchKernelGGL(mol_unique_finish_kernel, dim3(gi_cdiv(G, 256)), dim3(256), 0, st, (const int*)slot_of,
                       (const unsigned*)minidx, status, G, rep, unique, counts);
    return gi_launch_status();
}

extern "C" int gi_mol_seen_add(int G, const unsigned long long* key, const int* status, const int* rep,
                               unsigned long long* table, long long capacity, int* info, int* is_new, void* stream) {
    (void)hipGetLastError();
    if (G < 0 || capacity < 1 || capacity > (1ll << 40) || (capacity & (capacity - 1)) != 0) return GI_EINVAL;
    if (G == 0) return 0;
    if (!key || !status || !rep || !table || !info || !is_new) return GI_EINVAL;
    hipLaunchKernelGGL(mol_seen_kernel, dim3(gi_cdiv(G, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)key,
                       status, rep, G, (u64*)table, (u64)capacity - 1, info, is_new);
    return gi_launch_status();
}
