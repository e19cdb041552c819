// Node reordering on the device (gfx950): what `PreprocessingGraph.node_remap` (MolecularGraph.py:435-461) does
// after it has a node ranking — `breadth_first_search` / `depth_first_search` (:328-433) from node rank[0], then
// `reorder_nodes` (:592-614) and `pad_graph_representation` (:616-633) — for M molecules in one launch, so that a
// loader can draw a fresh decoding route per molecule per epoch in front of gi_route_plan / gi_route_expand.
//
// route_reorder_kernel, one 256-lane workgroup per molecule:
//   1  all waves read the molecule (gi_for_each_nonzero of gi_molread.h: 16-byte granules where the address allows,
//      bytes at the ragged ends), check it and build the adjacency ("any bond type set") as N bit rows of 128 bits
//      in LDS;
//   2  the ranking: the caller's (checked to be a permutation of 0..n-1) or drawn from (seed, epoch, molecule id):
//      key_i = mix64(s ^ (id << 8 | i)), rank_i = #{j : (key_j, j) < (key_i, i)};
//   3  wave 0 searches with `visited` and the frontier as wave-uniform 128-bit masks.
//      BFS: the next level is the OR of the frontier's rows (one butterfly per level) minus `visited`; a node's place
//      inside the level is the popcount of the level's bits below it, i.e. ASCENDING INPUT INDEX.  (The reference
//      extends its list by a Python set, whose iteration order is ascending only while the ids stay below the set's
//      table size; that accident is not reproduced.  The level sets are the reference's.)
//      DFS: the reference's loop — candidates = unvisited neighbours of order[pos]; none: pos -= 1 (by POSITION in the
//      visit list, not to the DFS parent); else append the one of highest rank (one lane-max) and pos = its place.
//      `visited` only grows, so a position found without candidates stays so: a mask of the still-live positions
//      lets the backward step jump to the next live one instead of re-testing the dead ones;
//   4  all waves gather nodes' = nodes[order], edges' = edges[order][:, order] (zero padded) and store them, again in
//      16-byte pieces between the ragged ends of the molecule's byte range (store_bytes of gi_molread.h).
// Every loop is bounded by the dims whatever the data holds: BFS runs at most N levels, DFS at most 2 N steps (each
// step appends a node or retires a position), every index is < N.  A molecule that fails a check is copied through
// unchanged with its GI_ROUTE_ERR_* bits in mol_err[m] and the identity in order[m].
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;                          // 128: a bit row is two 64-bit words

struct Mask {                                               // 128 bits
    u64 lo, hi;
    __device__ __forceinline__ bool any() const { return (lo | hi) != 0; }
    __device__ __forceinline__ bool test(int i) const { return ((i < 64 ? lo >> i : hi >> (i - 64)) & 1) != 0; }
    __device__ __forceinline__ void set(int i) { if (i < 64) lo |= 1ull << i; else hi |= 1ull << (i - 64); }
    __device__ __forceinline__ void clear(int i) { if (i < 64) lo &= ~(1ull << i); else hi &= ~(1ull << (i - 64)); }
    __device__ __forceinline__ int count() const { return __popcll(lo) + __popcll(hi); }
    // bits below i set, 0 <= i <= 128
    static __device__ __forceinline__ Mask below(int i) {
        Mask m;
        m.lo = i >= 64 ? ~0ull : (1ull << i) - 1;
        m.hi = i <= 64 ? 0ull : i >= 128 ? ~0ull : (1ull << (i - 64)) - 1;
        return m;
    }
    __device__ __forceinline__ Mask operator&(const Mask& o) const { return Mask{lo & o.lo, hi & o.hi}; }
    __device__ __forceinline__ Mask andnot(const Mask& o) const { return Mask{lo & ~o.lo, hi & ~o.hi}; }
    __device__ __forceinline__ int highest() const {         // index of the highest set bit, -1 if none
        return hi ? 127 - __clzll((long long)hi) : lo ? 63 - __clzll((long long)lo) : -1;
    }
};

__device__ __forceinline__ Mask wave_or(Mask x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        x.lo |= (u64)__shfl_xor((long long)x.lo, s);
        x.hi |= (u64)__shfl_xor((long long)x.hi, s);
    }
    return x;
}

template <int MODE>                                         // GI_ROUTE_BFS / GI_ROUTE_DFS
__global__ __launch_bounds__(NT) void route_reorder_kernel(const i8* __restrict__ nodes, const i8* __restrict__ edges,
                                                           int N, int Fn, int Fe, const int* __restrict__ rank_in,
                                                           u64 seed, u64 epoch, const long long* __restrict__ mol_ids,
                                                           i8* __restrict__ out_nodes, i8* __restrict__ out_edges,
                                                           int* __restrict__ order_out, int* __restrict__ mol_err) {
    __shared__ unsigned adj[MAXN][4];                       // bit j of row i: a bond between i and j
    __shared__ u64 key[MAXN];
    __shared__ int rank[MAXN], order[MAXN];
    __shared__ unsigned present[4], seen[4];
    __shared__ int err_sh, rank_err_sh;                     // structure and search / the ranking
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int len_n = N * Fn, len_e = N * N * Fe;
    const i8* nd = nodes + (size_t)m * len_n;
    const i8* ed = edges + (size_t)m * len_e;
    for (int i = tid; i < MAXN * 4; i += NT) (&adj[0][0])[i] = 0u;
    if (tid < 4) { present[tid] = 0u; seen[tid] = 0u; }
    if (tid == 0) { err_sh = 0; rank_err_sh = 0; }
    __syncthreads();

    // ---- 1: read and check -------------------------------------------------------------------------------
    int err = 0;
    gi_for_each_nonzero(nd, len_n, tid, [&](int o, i8 v) {
        if (v != 1) err |= GI_ROUTE_ERR_VALUE;
        const int i = o / Fn;
        atomicOr(&present[i >> 5], 1u << (i & 31));
    });
    gi_for_each_nonzero(ed, len_e, tid, [&](int o, i8 v) {
        if (v != 1) err |= GI_ROUTE_ERR_VALUE;
        const int e = o / Fe, t = o - e * Fe, i = e / N, j = e - i * N;
        if (ed[((size_t)j * N + i) * Fe + t] != v) err |= GI_ROUTE_ERR_ASYMMETRIC;   // every mismatch has a set side
        atomicOr(&adj[i][j >> 5], 1u << (j & 31));
    });
    __syncthreads();
    const Mask pres{present[0] | (u64)present[1] << 32, present[2] | (u64)present[3] << 32};
    const int n = pres.count();
    if (n == 0) err |= GI_ROUTE_ERR_EMPTY;
    if (pres.lo != Mask::below(n).lo || pres.hi != Mask::below(n).hi) err |= GI_ROUTE_ERR_PADDING;
    if (tid < N) {
        const int i = tid;
        Mask row{adj[i][0] | (u64)adj[i][1] << 32, adj[i][2] | (u64)adj[i][3] << 32};
        if (row.any() && (i >= n || row.test(i) || row.andnot(Mask::below(n)).any())) err |= GI_ROUTE_ERR_PADDING;
    }

    if (err) atomicOr(&err_sh, err);
    __syncthreads();

    // ---- 2: the ranking (of a molecule that passed: n means nothing otherwise) ----------------------------
    const bool sound = err_sh == 0;                         // uniform; err_sh is not written again before the search
    if (!sound) {
    } else if (rank_in) {
        if (tid < n) {
            const int r = rank_in[(size_t)m * N + tid];
            const unsigned bit = 1u << (r & 31);
            rank[tid] = r;
            if (r < 0 || r >= n || (atomicOr(&seen[(r >> 5) & 3], bit) & bit)) rank_err_sh = GI_ROUTE_ERR_RANK;
        }
    } else {
        const u64 s = mix64(mix64(seed) + epoch);
        const u64 id = mol_ids ? (u64)mol_ids[m] : (u64)m;
        if (tid < N) key[tid] = mix64(s ^ ((id << 8) | (u64)tid));
        __syncthreads();
        if (tid < n) {
            const u64 k = key[tid];
            int r = 0;
            for (int j = 0; j < n; ++j) r += key[j] < k || (key[j] == k && j < tid);
            rank[tid] = r;
        }
    }
    __syncthreads();

    // ---- 3: the search (wave 0; everything below is wave-uniform) ---------------------------------------
    if (tid < 64 && sound && rank_err_sh == 0) {
        const int start = rank[0];                          // the rank VALUE of node 0, used as a node index (:455)
        const int i0 = lane, i1 = lane + 64;                // the two nodes of this lane
        const Mask row0{adj[i0][0] | (u64)adj[i0][1] << 32, adj[i0][2] | (u64)adj[i0][3] << 32};
        const Mask row1{adj[i1][0] | (u64)adj[i1][1] << 32, adj[i1][2] | (u64)adj[i1][3] << 32};
        Mask visited{0, 0};
        visited.set(start);
        order[0] = start;                                   // every lane stores the same value: no lane reads
                                                            // order[] before it has written that entry itself
        int cnt = 1, bad = 0;
        if (MODE == GI_ROUTE_BFS) {
            Mask frontier = visited;
            for (int level = 0; level < N && cnt < n; ++level) {
                Mask next{0, 0};
                if (frontier.test(i0)) next = row0;
                if (frontier.test(i1)) { next.lo |= row1.lo; next.hi |= row1.hi; }
                next = wave_or(next).andnot(visited);
                if (!next.any()) { bad = GI_ROUTE_ERR_CONNECT; break; }
                if (next.test(i0)) order[cnt + (next & Mask::below(i0)).count()] = i0;
                if (next.test(i1)) order[cnt + (next & Mask::below(i1)).count()] = i1;
                cnt += next.count();
                visited.lo |= next.lo; visited.hi |= next.hi;
                frontier = next;
            }
        } else {
            const int r0 = i0 < n ? rank[i0] * MAXN + i0 : -1, r1 = i1 < n ? rank[i1] * MAXN + i1 : -1;
            Mask live{1, 0};                                // positions of `order` that may still have candidates
            int pos = 0;
            for (int step = 0; step < 2 * N && cnt < n; ++step) {
                const int p = (live & Mask::below(pos + 1)).highest();
                if (p < 0) { bad = GI_ROUTE_ERR_CONNECT; break; }     // the reference's pos - 1 wraps round here
                const int at = order[p];
                const Mask cand = Mask{adj[at][0] | (u64)adj[at][1] << 32,
                                       adj[at][2] | (u64)adj[at][3] << 32}.andnot(visited);
                if (!cand.any()) { live.clear(p); pos = p - 1; continue; }
                const int best = wave_max(max(cand.test(i0) ? r0 : -1, cand.test(i1) ? r1 : -1)) & (MAXN - 1);
                order[cnt] = best;
                visited.set(best);
                live.set(cnt);
                pos = cnt++;
            }
        }
        if (cnt < n && !bad) bad = GI_ROUTE_ERR_CONNECT;    // not reached: the loops above end on cnt == n or `bad`
        if (bad && lane == 0) err_sh = bad;
    }
    __syncthreads();

    // ---- 4: gather and store -----------------------------------------------------------------------------
    const int e_all = err_sh | rank_err_sh;
    const int n_out = e_all ? N : n;                        // a molecule that failed is copied through
    if (e_all) {                                            // uniform branch
        for (int i = tid; i < N; i += NT) order[i] = i;
        __syncthreads();
    }
    if (tid == 0) mol_err[m] = e_all;
    if (order_out)
        for (int i = tid; i < N; i += NT) order_out[(size_t)m * N + i] = i < n_out ? order[i] : -1;
    store_bytes(out_nodes + (size_t)m * len_n, len_n, tid, N, 1, Fn,
                [&](int a, int) { return a < n_out ? order[a] * Fn : -1; },
                [&](int s, int f) { return (int)nd[s + f]; });
    store_bytes(out_edges + (size_t)m * len_e, len_e, tid, N, N, Fe,
                [&](int a, int b) {
                    if (a >= n_out || b >= n_out) return -1;
                    const int i = order[a], j = order[b];      // a set byte has its adjacency bit, whatever its value
                    return (adj[i][j >> 5] >> (j & 31)) & 1u ? (i * N + j) * Fe : -1;
                },
                [&](int s, int t) { return (int)ed[s + t]; });
}

}  // namespace

extern "C" int gi_route_reorder(int M, int N, int Fn, int Fe, const signed char* nodes, const signed char* edges,
                                const int* rank, unsigned long long seed, unsigned long long epoch,
                                const long long* mol_ids, int mode, signed char* out_nodes, signed char* out_edges,
                                int* order, int* mol_err, void* stream) {
    (void)hipGetLastError();
    if (M < 0 || N < 1 || Fn < 1 || Fe < 1 || (mode != GI_ROUTE_BFS && mode != GI_ROUTE_DFS)) return GI_EINVAL;
    if (N > GI_MAX_NODES || Fe > GI_MAX_GROUPS || (long long)N * Fn > (1 << 24)) return GI_ELIMIT;
    if (M == 0) return 0;
    if (!nodes || !edges || !out_nodes || !out_edges || !mol_err) return GI_EINVAL;
    if (nodes == out_nodes || edges == out_edges) return GI_EINVAL;             // not in place
    const hipStream_t st = (hipStream_t)stream;
#define GI_ROUTE_REORDER(MODE_)                                                                                  \
    hipLaunchKernelGGL((route_reorder_kernel<MODE_>), dim3(M), dim3(NT), 0, st, nodes, edges, N, Fn, Fe, rank,   \
                       (u64)seed, (u64)epoch, mol_ids, out_nodes, out_edges, order, mol_err)
    if (mode == GI_ROUTE_BFS) GI_ROUTE_REORDER(GI_ROUTE_BFS); else GI_ROUTE_REORDER(GI_ROUTE_DFS);
#undef GI_ROUTE_REORDER
    return gi_launch_status();
}
