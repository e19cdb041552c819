// Growth step of graph generation (gfx950): the bookkeeping of one GraphGenerator.build_graphs round —
// properly_terminated, copy_terminated_graphs, apply_actions, reset_graphs and the dummy graph's restore
// (GraphGenerator.py:126-157, 211-465) — from gi_sample_actions' raw per-graph action / likelihood / flags, in place on
// the generator's tensors.  The reference lays the draw out as index tuples through boolean masks, `nonzero` and
// `len(...)`, each a read-back; here nothing leaves the device, and a whole round (forward, draw, growth) can be
// recorded into one hipGraph.
//
// Three launches in stream order, so that every reader of the round's n and r sees the values of the round's entry:
//   1. grow_scan_kernel (one workgroup): ranks inside S, |T|, |S|, every index check, the round's go / error decision,
//      properly_terminated;
//   2. grow_apply_kernel (one workgroup per graph): copy to the generated rows, apply, reset, restore graph 0;
//   3. grow_commit_kernel (one thread): n += |S|, r += 1 or the error bits; the mapped host mirror.
// Workspace in desc.state: [0] n, [1] r, [2] target, [3] error (persistent); [4] go, [5] |S|, [6] |T \ {0}|,
// [7] |T|, [8] new error bits (this round's); [GI_GROW_STATE_WORDS + g] = graph g's slot: k >= 0 at position k of
// T \ {0}, -2 - k at position k of I \ {0}, -1 outside S.
//
// gi_grow_graphs_rl runs the same three launches with the RL fields of GrowArgs set: the prior's likelihood stream
// beside the agent's (d.likelihoods / d.gen_likelihoods / d.likelihood), and the trajectory record of every generated
// row (source graph, first and last round) from the per-graph start rounds in state[GI_GROW_STATE_WORDS + B + g].
// gi_grow_traj_gather / gi_grow_traj_scatter rebuild the generated likelihood rows from the per-round likelihoods with
// that record, and take the gradient back, for the autograd of the RL loop.
//
// gi_grow_graphs_seeded / gi_grow_graphs_rl_seeded run the same three launches with a seed bank (SeedArgs): a graph
// written out in the round restarts from seed (B - 1 + row) mod S of the bank instead of from the empty graph, and
// gen_seed[row] receives the seed it was grown from, kept per slot in state[GI_GROW_STATE_WORDS + 2 B + g].  The bank
// is int8 and tightly packed, so a seed starts at any byte address: it is read one byte per element.
// gi_grow_seed_init writes the first fill.
#include "gi_common.h"

namespace {

constexpr int SCAN_THREADS = 1024;           // 16 waves of 64
constexpr int APPLY_THREADS = 256;
constexpr int SLOT_NONE = -1;

struct GrowArgs {
    gi_grow_desc d;
    int A;                                   // add actions per node: prod(group) * Fe
    // gi_grow_graphs_rl only (NULL in gi_grow_graphs): the prior's stream, the trajectory record, the start rounds
    float* p_likelihoods;                    // [B, L]
    float* p_gen;                            // [C, L]
    const float* p_like;                     // [B]
    int* traj;                               // [3, C]
    int* start;                              // [B], in state
};

// the seed bank of the seeded entry points (gi_grow_seed_desc) and the per-slot seed indices in state
struct SeedArgs {
    const signed char* nodes;                // [S, N, Fn]
    const signed char* edges;                // [S, N, N, Fe]
    const signed char* n_nodes;              // [S]
    int* gen_seed;                           // [C] or NULL
    int* slot_seed;                          // [B], in state
    int S;
};

__device__ __forceinline__ long long node_off(const gi_grow_desc& d, int g) { return (long long)g * d.N * d.Fn; }
__device__ __forceinline__ long long edge_off(const gi_grow_desc& d, int g) {
    return (long long)g * d.N * d.N * d.Fe;
}

__global__ __launch_bounds__(SCAN_THREADS) void grow_scan_kernel(GrowArgs a) {
    const gi_grow_desc& d = a.d;
    __shared__ int wsum[SCAN_THREADS / 64];
    __shared__ int bits_s;
    __shared__ int sh[4];                    // go, n, |T|
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int* slot = d.state + GI_GROW_STATE_WORDS;
    if (tid == 0) bits_s = 0;
    __syncthreads();
    int carry_t = 0, carry_i = 0, graph0_term = 0;
    // packed counts: terminated (g != 0) in the low 16 bits, invalid (g != 0) in the high ones; a chunk of 1024 fits
    for (int base = 0; base < d.B; base += SCAN_THREADS) {
        const int g = base + tid;
        int is_t = 0, is_i = 0, bad = 0;
        if (g < d.B) {
            const int kind = d.action[4 * g + 0], to = d.action[4 * g + 1], rem = d.action[4 * g + 2],
                      from = d.action[4 * g + 3];
            const int inv = d.flags[g] & 1;
            const int nn = d.n_nodes[g];
            if (kind < 0 || kind > 2) bad |= GI_GROW_ERR_ACTION;
            if (kind == 2 && inv) bad |= GI_GROW_ERR_ACTION;
            if (kind == 0 && (to < 0 || to >= d.N || rem < 0 || rem >= a.A || from < 0 || from >= d.N))
                bad |= GI_GROW_ERR_ACTION;
            if (kind == 1 && (to < 0 || to >= d.N || rem < 0 || rem >= d.Fe || from < -1 || from >= d.N))
                bad |= GI_GROW_ERR_ACTION;
            // an add that survives the round (not reset, not the restored graph 0) must not wrap the int8 count
            if (kind == 0 && !inv && g != 0 && nn >= 127) bad |= GI_GROW_ERR_NNODES;
            if (g == 0 && kind == 2) graph0_term = 1;
            is_t = (kind == 2 && g != 0);
            is_i = (inv && g != 0);
        }
        if (bad) atomicOr(&bits_s, bad);
        const int v = is_t | (is_i << 16);
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            if (w < wid) woff += wsum[w];
            tot += wsum[w];
        }
        const int excl = woff + x - v;
        if (g < d.B)
            slot[g] = is_t ? carry_t + (excl & 0xffff) : (is_i ? -2 - (carry_i + (excl >> 16)) : SLOT_NONE);
        carry_t += tot & 0xffff;
        carry_i += tot >> 16;
        __syncthreads();                     // wsum is reused by the next chunk
    }
    if (graph0_term) atomicOr(&bits_s, 1 << 30);   // (graph 0 is in the first chunk: carried through bits_s)
    __syncthreads();
    if (tid == 0) {
        const int n = d.state[0], r = d.state[1], target = d.state[2], err = d.state[3];
        const int n_s = carry_t + carry_i;
        const int n_t = carry_t + ((bits_s >> 30) & 1);
        int bits = bits_s & ~(1 << 30);
        int go = 0;
        if (n < target && err == 0) {
            if (r >= d.L) bits |= GI_GROW_ERR_ROUND;
            if ((long long)n + n_s > d.C) bits |= GI_GROW_ERR_CAPACITY;
            go = bits == 0;
        } else {
            bits = 0;                        // frozen: this round neither writes nor reports
        }
        d.state[4] = go;
        d.state[5] = n_s;
        d.state[6] = carry_t;
        d.state[7] = n_t;
        d.state[8] = bits;
        sh[0] = go; sh[1] = n; sh[2] = n_t;
    }
    __syncthreads();
    if (!sh[0]) return;
    const int n = sh[1], end = min(n + sh[2], d.C);           // torch clips the slice at C (:127)
    for (int i = n + tid; i < end; i += SCAN_THREADS) d.properly_terminated[i] = 1;
}

template <bool SEEDED>
__device__ __forceinline__ void grow_apply(const GrowArgs& a, const SeedArgs& sd) {
    const gi_grow_desc& d = a.d;
    const int* st = d.state;
    if (!st[4]) return;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = st[0], r = st[1], n_t0 = st[6];
    const int s = st[GI_GROW_STATE_WORDS + g];
    const float like = d.likelihood[g];
    const int NF = d.N * d.Fn, NNF = d.N * d.N * d.Fe;
    float* nodes = d.nodes + node_off(d, g);
    float* edges = d.edges + edge_off(d, g);
    float* lrow = d.likelihoods + (long long)g * d.L;
    if (s != SLOT_NONE) {
        // copy (:365-383) with likelihoods[g, r] = likelihood[g], then the reset (:430-465): the action applied in
        // between (:211-338) only touches what the reset clears
        const int k = s >= 0 ? s : n_t0 + (-2 - s);
        const long long row = (long long)n + k;
        float* gn = d.gen_nodes + (long long)row * NF;
        float* ge = d.gen_edges + (long long)row * NNF;
        float* gl = d.gen_likelihoods + row * d.L;
        int next = 0;
        if (SEEDED) {
            // the restart: seed (B - 1 + row) mod S, one byte per element (a seed starts at any byte address)
            next = (int)(((long long)d.B - 1 + row) % sd.S);
            const signed char* sn = sd.nodes + (long long)next * NF;
            const signed char* se = sd.edges + (long long)next * NNF;
            for (int i = tid; i < NF; i += APPLY_THREADS) { gn[i] = nodes[i]; nodes[i] = (float)sn[i]; }
            for (int i = tid; i < NNF; i += APPLY_THREADS) { ge[i] = edges[i]; edges[i] = (float)se[i]; }
        } else {
            for (int i = tid; i < NF; i += APPLY_THREADS) { gn[i] = nodes[i]; nodes[i] = 0.f; }
            for (int i = tid; i < NNF; i += APPLY_THREADS) { ge[i] = edges[i]; edges[i] = 0.f; }
        }
        for (int j = tid; j < d.L; j += APPLY_THREADS) { gl[j] = j == r ? like : lrow[j]; lrow[j] = 0.f; }
        if (a.p_likelihoods) {
            const float plike = a.p_like[g];
            float* prow = a.p_likelihoods + (long long)g * d.L;
            float* pg = a.p_gen + row * d.L;
            for (int j = tid; j < d.L; j += APPLY_THREADS) { pg[j] = j == r ? plike : prow[j]; prow[j] = 0.f; }
        }
        if (tid == 0) {
            d.gen_n_nodes[row] = d.n_nodes[g];
            if (SEEDED) {                    // (only block g touches slot_seed[g])
                d.n_nodes[g] = sd.n_nodes[next];
                if (sd.gen_seed) sd.gen_seed[row] = sd.slot_seed[g];
                sd.slot_seed[g] = next;
            } else {
                d.n_nodes[g] = 0;
            }
            if (a.start) {                   // (only block g touches start[g])
                if (a.traj) {
                    a.traj[row] = g;
                    a.traj[d.C + row] = a.start[g];
                    a.traj[2LL * d.C + row] = r;
                }
                a.start[g] = r + 1;
            }
        }
        return;
    }
    // every other graph applies its action; graph 0 is then restored
    if (g == 0)
        for (int i = tid; i < NF; i += APPLY_THREADS) nodes[i] = 1.f;   // (what an add would set is 1 already)
    if (tid != 0) return;
    const int kind = d.action[4 * g + 0], to = d.action[4 * g + 1], rem = d.action[4 * g + 2],
              from = d.action[4 * g + 3];
    const int N = d.N, Fe = d.Fe;
    if (kind == 0) {                                              // add (:264-317)
        const int nn = d.n_nodes[g];
        const int bt = rem % Fe;
        if (g != 0) {
            int q = rem / Fe, off = d.Fn;
            for (int j = d.n_groups - 1; j >= 0; --j) {          // unravel over the node-feature groups, last fastest
                const int size = d.group[j];
                off -= size;
                nodes[from * d.Fn + off + q % size] = 1.f;
                q /= size;
            }
        }
        if (nn != 0) {                                            // no bond for a first atom (:304-311)
            edges[((long long)to * N + from) * Fe + bt] = 1.f;
            edges[((long long)from * N + to) * Fe + bt] = 1.f;
        }
        d.n_nodes[g] = g == 0 ? 1 : (signed char)(nn + 1);       // :314 (graph 0: restored, :463)
        lrow[r] = like;                                           // :315
        if (a.p_likelihoods) a.p_likelihoods[(long long)g * d.L + r] = a.p_like[g];
    } else if (kind == 1) {                                       // connect (:319-337)
        const int f = from < 0 ? from + N : from;                 // torch's wrap of -1
        edges[((long long)f * N + to) * Fe + rem] = 1.f;
        edges[((long long)to * N + f) * Fe + rem] = 1.f;
        lrow[r] = like;
        if (a.p_likelihoods) a.p_likelihoods[(long long)g * d.L + r] = a.p_like[g];
    }
    if (g == 0) {
        edges[0] = 1.f;                                           // :462
        d.n_nodes[0] = 1;
    }
}

__global__ __launch_bounds__(APPLY_THREADS) void grow_apply_kernel(GrowArgs a) { grow_apply<false>(a, SeedArgs{}); }

__global__ __launch_bounds__(APPLY_THREADS) void grow_apply_seeded_kernel(GrowArgs a, SeedArgs sd) {
    grow_apply<true>(a, sd);
}

// the first fill: slot g >= 1 takes seed (g - 1) mod S; slot 0 (the dummy graph) is left as it is
__global__ __launch_bounds__(APPLY_THREADS) void grow_seed_init_kernel(GrowArgs a, SeedArgs sd) {
    const gi_grow_desc& d = a.d;
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g == 0) {
        if (tid == 0) sd.slot_seed[0] = -1;
        return;
    }
    const int NF = d.N * d.Fn, NNF = d.N * d.N * d.Fe;
    const int seed = (g - 1) % sd.S;
    const signed char* sn = sd.nodes + (long long)seed * NF;
    const signed char* se = sd.edges + (long long)seed * NNF;
    float* nodes = d.nodes + node_off(d, g);
    float* edges = d.edges + edge_off(d, g);
    float* lrow = d.likelihoods + (long long)g * d.L;
    for (int i = tid; i < NF; i += APPLY_THREADS) nodes[i] = (float)sn[i];
    for (int i = tid; i < NNF; i += APPLY_THREADS) edges[i] = (float)se[i];
    for (int j = tid; j < d.L; j += APPLY_THREADS) lrow[j] = 0.f;
    if (a.p_likelihoods) {
        float* prow = a.p_likelihoods + (long long)g * d.L;
        for (int j = tid; j < d.L; j += APPLY_THREADS) prow[j] = 0.f;
    }
    if (tid == 0) {
        d.n_nodes[g] = sd.n_nodes[seed];
        sd.slot_seed[g] = seed;
    }
}

__global__ __launch_bounds__(64) void grow_commit_kernel(int* state, int* host_state) {
    if (threadIdx.x != 0) return;
    if (state[4]) {
        state[0] += state[5];
        state[1] += 1;
    } else {
        state[3] |= state[8];
    }
    if (host_state) {
        volatile int* h = host_state;
        h[0] = state[0]; h[1] = state[1]; h[2] = state[2]; h[3] = state[3];
        __threadfence_system();
    }
}

}  // namespace

extern "C" int gi_grow_state_words(int B) { return B < 0 ? GI_EINVAL : GI_GROW_STATE_WORDS + B; }

namespace {

// gi_grow_desc's checks; fills a (the RL fields NULL)
int grow_args(const gi_grow_desc& d, GrowArgs& a) {
    if (d.B <= 0 || d.N <= 0 || d.Fn <= 0 || d.Fe <= 0 || d.L <= 0 || d.C <= 0) return GI_EINVAL;
    if (d.N > GI_MAX_NODES || d.n_groups < 1 || d.n_groups > GI_GROW_MAX_GROUPS) return GI_ELIMIT;
    if (!d.nodes || !d.edges || !d.n_nodes || !d.likelihoods || !d.gen_nodes || !d.gen_edges || !d.gen_n_nodes ||
        !d.gen_likelihoods || !d.properly_terminated || !d.action || !d.likelihood || !d.flags || !d.state)
        return GI_EINVAL;
    long long A = d.Fe, sum = 0;
    for (int j = 0; j < d.n_groups; ++j) {
        if (d.group[j] <= 0) return GI_EINVAL;
        A *= d.group[j];
        sum += d.group[j];
        if (A > 0x7fffffffLL) return GI_ELIMIT;
    }
    if (sum != d.Fn) return GI_EINVAL;       // every add writes one feature per group: the groups tile the node row
    if ((long long)d.N * d.N * d.Fe > 0x7fffffffLL) return GI_ELIMIT;
    a = GrowArgs{};
    a.d = d;
    a.A = (int)A;
    return 0;
}

// gi_grow_seed_desc's checks; fills sd (slot_seed from d.state)
int seed_args(const gi_grow_desc& d, const gi_grow_seed_desc* seeds, SeedArgs& sd) {
    if (!seeds || seeds->S < 1 || !seeds->nodes || !seeds->edges || !seeds->n_nodes) return GI_EINVAL;
    if ((long long)seeds->S * d.N * d.N * d.Fe > 0x7fffffffffffLL) return GI_ELIMIT;
    sd.nodes = seeds->nodes;
    sd.edges = seeds->edges;
    sd.n_nodes = seeds->n_nodes;
    sd.gen_seed = seeds->gen_seed;
    sd.slot_seed = d.state + GI_GROW_STATE_WORDS + 2LL * d.B;
    sd.S = seeds->S;
    return 0;
}

int grow_launch(const GrowArgs& a, void* stream, const SeedArgs* sd = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grow_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, a);
    if (sd)
        hipLaunchKernelGGL(grow_apply_seeded_kernel, dim3(a.d.B), dim3(APPLY_THREADS), 0, st, a, *sd);
    else
        hipLaunchKernelGGL(grow_apply_kernel, dim3(a.d.B), dim3(APPLY_THREADS), 0, st, a);
    hipLaunchKernelGGL(grow_commit_kernel, dim3(1), dim3(64), 0, st, a.d.state, a.d.host_state);
    return gi_launch_status();
}

constexpr int TRAJ_THREADS = 256;

// one workgroup per generated row k: gen[k, c] for every column c, both sides
__global__ __launch_bounds__(TRAJ_THREADS) void traj_gather_kernel(int n, int R, int B, int C, int L,
                                                                   const int* __restrict__ traj,
                                                                   const float* __restrict__ like_a,
                                                                   const float* __restrict__ like_p,
                                                                   float* __restrict__ gen_a, float* __restrict__ gen_p) {
    const int k = blockIdx.x;
    int g = -1, lo = 1, hi = 0;
    if (k < n) {
        g = traj[k]; lo = traj[C + k]; hi = min(traj[2 * C + k], R - 1);
        if (g < 0 || g >= B) lo = 1, hi = 0;                      // (never recorded so: nothing read out of range)
    }
    for (int c = threadIdx.x; c < L; c += TRAJ_THREADS) {
        const bool in = c >= lo && c <= hi;
        const long long src = (long long)c * B + g;
        if (gen_a) gen_a[(long long)k * L + c] = in ? like_a[src] : 0.f;
        if (gen_p) gen_p[(long long)k * L + c] = in ? like_p[src] : 0.f;
    }
}

// one workgroup per round c: zero d[c, :], then every row covering c writes its (c, graph) element
__global__ __launch_bounds__(TRAJ_THREADS) void traj_scatter_kernel(int n, int B, int C,
                                                                    const int* __restrict__ traj,
                                                                    const float* __restrict__ g_a, int ldg_a,
                                                                    const float* __restrict__ g_p, int ldg_p,
                                                                    float* __restrict__ d_a, float* __restrict__ d_p) {
    const int c = blockIdx.x;
    for (int g = threadIdx.x; g < B; g += TRAJ_THREADS) {
        if (d_a) d_a[(long long)c * B + g] = 0.f;
        if (d_p) d_p[(long long)c * B + g] = 0.f;
    }
    __syncthreads();                         // (the zeros are visible to the workgroup's own writes below)
    for (int k = threadIdx.x; k < n; k += TRAJ_THREADS) {
        const int g = traj[k];
        if (g < 0 || g >= B || c < traj[C + k] || c > traj[2 * C + k]) continue;
        if (d_a) d_a[(long long)c * B + g] = g_a[(long long)k * ldg_a + c];
        if (d_p) d_p[(long long)c * B + g] = g_p[(long long)k * ldg_p + c];
    }
}

}  // namespace

extern "C" int gi_grow_graphs(const gi_grow_desc* desc, void* stream) {
    (void)hipGetLastError();
    if (!desc) return GI_EINVAL;
    GrowArgs a;
    const int rc = grow_args(*desc, a);
    if (rc) return rc;
    return grow_launch(a, stream);
}

extern "C" int gi_grow_rl_state_words(int B) { return B < 0 ? GI_EINVAL : GI_GROW_STATE_WORDS + 2 * B; }

namespace {

// gi_grow_rl_desc's checks on top of grow_args'
int grow_args_rl(const gi_grow_rl_desc* desc, GrowArgs& a) {
    if (!desc) return GI_EINVAL;
    const int rc = grow_args(desc->base, a);
    if (rc) return rc;
    const int n_prior = !!desc->prior_likelihoods + !!desc->gen_prior_likelihoods + !!desc->prior_likelihood;
    if (n_prior != 0 && n_prior != 3) return GI_EINVAL;
    if ((long long)3 * desc->base.C > 0x7fffffffLL) return GI_ELIMIT;
    a.p_likelihoods = desc->prior_likelihoods;
    a.p_gen = desc->gen_prior_likelihoods;
    a.p_like = desc->prior_likelihood;
    a.traj = desc->traj;
    a.start = desc->base.state + GI_GROW_STATE_WORDS + desc->base.B;
    return 0;
}

}  // namespace

extern "C" int gi_grow_graphs_rl(const gi_grow_rl_desc* desc, void* stream) {
    (void)hipGetLastError();
    GrowArgs a;
    const int rc = grow_args_rl(desc, a);
    if (rc) return rc;
    return grow_launch(a, stream);
}

extern "C" int gi_grow_seeded_state_words(int B) { return B < 0 ? GI_EINVAL : GI_GROW_STATE_WORDS + 3 * B; }

extern "C" int gi_grow_seed_init(const gi_grow_desc* desc, const gi_grow_seed_desc* seeds, float* prior_likelihoods,
                                 void* stream) {
    (void)hipGetLastError();
    if (!desc) return GI_EINVAL;
    const gi_grow_desc& d = *desc;
    if (d.B <= 0 || d.N <= 0 || d.Fn <= 0 || d.Fe <= 0 || d.L <= 0) return GI_EINVAL;
    if (d.N > GI_MAX_NODES) return GI_ELIMIT;
    if ((long long)d.N * d.N * d.Fe > 0x7fffffffLL || (long long)d.N * d.Fn > 0x7fffffffLL) return GI_ELIMIT;
    if (!d.nodes || !d.edges || !d.n_nodes || !d.likelihoods || !d.state) return GI_EINVAL;
    GrowArgs a{};
    a.d = d;
    a.p_likelihoods = prior_likelihoods;
    SeedArgs sd;
    const int rc = seed_args(d, seeds, sd);
    if (rc) return rc;
    hipLaunchKernelGGL(grow_seed_init_kernel, dim3(d.B), dim3(APPLY_THREADS), 0, (hipStream_t)stream, a, sd);
    return gi_launch_status();
}

extern "C" int gi_grow_graphs_seeded(const gi_grow_desc* desc, const gi_grow_seed_desc* seeds, void* stream) {
    (void)hipGetLastError();
    if (!desc) return GI_EINVAL;
    GrowArgs a;
    int rc = grow_args(*desc, a);
    if (rc) return rc;
    SeedArgs sd;
    rc = seed_args(a.d, seeds, sd);
    if (rc) return rc;
    return grow_launch(a, stream, &sd);
}

extern "C" int gi_grow_graphs_rl_seeded(const gi_grow_rl_desc* desc, const gi_grow_seed_desc* seeds, void* stream) {
    (void)hipGetLastError();
    GrowArgs a;
    int rc = grow_args_rl(desc, a);
    if (rc) return rc;
    SeedArgs sd;
    rc = seed_args(a.d, seeds, sd);
    if (rc) return rc;
    return grow_launch(a, stream, &sd);
}

extern "C" int gi_grow_traj_gather(int n, int R, int B, int C, int L, const int* traj, const float* like_a,
                                   const float* like_p, float* gen_a, float* gen_p, void* stream) {
    (void)hipGetLastError();
    if (n < 0 || R < 0 || B <= 0 || C <= 0 || L <= 0 || n > C || R > L || !traj) return GI_EINVAL;
    if (!gen_a != !like_a || !gen_p != !like_p || (!gen_a && !gen_p)) return GI_EINVAL;
    if ((long long)3 * C > 0x7fffffffLL) return GI_ELIMIT;
    hipLaunchKernelGGL(traj_gather_kernel, dim3(C), dim3(TRAJ_THREADS), 0, (hipStream_t)stream, n, R, B, C, L, traj,
                       like_a, like_p, gen_a, gen_p);
    return gi_launch_status();
}

extern "C" int gi_grow_traj_scatter(int n, int R, int B, int C, int L, const int* traj, const float* g_a, int ldg_a,
                                    const float* g_p, int ldg_p, float* d_a, float* d_p, void* stream) {
    (void)hipGetLastError();
    if (n < 0 || R < 0 || B <= 0 || C <= 0 || L <= 0 || n > C || R > L || !traj) return GI_EINVAL;
    if (!d_a != !g_a || !d_p != !g_p || (!d_a && !d_p)) return GI_EINVAL;
    if ((d_a && ldg_a < L) || (d_p && ldg_p < L)) return GI_EINVAL;
    if ((long long)3 * C > 0x7fffffffLL) return GI_ELIMIT;
    if (R == 0) return 0;
    hipLaunchKernelGGL(traj_scatter_kernel, dim3(R), dim3(TRAJ_THREADS), 0, (hipStream_t)stream, n, B, C, traj,
                       g_a, ldg_a, g_p, ldg_p, d_a, d_p);
    return gi_launch_status();
}
