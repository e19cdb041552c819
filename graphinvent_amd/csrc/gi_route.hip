// Decoding routes on the device (gfx950): from whole molecules to the training rows the reference's preprocessing
// writes — every `PreprocessingGraph.get_decoding_route_state(k)` (MolecularGraph.py:691-732) of every molecule, and
// the merge of identical subgraphs `DataProcesser.get_subgraphs` intends (DataProcesser.py:204-231).
//
// The route in closed form.  The reference truncates from the last node: its neighbours are listed bond type first,
// node index second (:502-506, :653-659), the LAST entry of the list is deleted, and the node goes with its last bond.
// While node i is the last one, every higher node is gone, so its neighbours are its lower ones; with d_i of them
// (c_i = d_i steps, c_0 = 1) node i's steps are start_i .. start_i + c_i - 1, start_i = 1 + sum_{i' > i} c_i', and the
// bond that is r-th in DESCENDING (type, index) order goes at step start_i + r.  Row k of the route is then a pure
// function of the molecule and k: nodes whose removal step is > k, bonds whose deletion step is > k, and the one hot
// APD entry of step k (f_conn[j, t] while the node keeps a bond, f_add[j, features.., t] with its last one).
//
// Launches:
//   route_plan_kernel    one 64-lane workgroup per molecule: the input checks, node / bond steps (a 16-bit word per
//                        node pair: step | type << 13, built in LDS), route length, per-node hash terms
//   route_scan_kernel    one workgroup: exclusive scan (row offsets of the molecules; later the kept rows' positions)
//   route_rows_kernel    one wave per row: (molecule, step) of the row, its hot APD index and a 64-bit hash of its
//                        (nodes, edges) content — a sum of per-set-bit terms, so equal graphs hash equal
//   route_expand_kernel  flat over the three outputs in aligned 16-byte pieces: each lane works out (row, offset) of its
//                        bytes and stores one uint4 (the row pitches are not multiples of 16)
//   merge: route_insert_kernel (one wave per row: probe an open-addressing table from the row's hash, claim an empty
//          slot or join the slot whose owner row is BYTE-identical, atomicMin of the row index into the slot),
//          route_rep_kernel, route_scan_kernel, route_gather_kernel, route_apd_kernel (exact integer adds).
// Which row of a class owns its table slot depends on timing; nothing visible does: the class is decided by the byte
// compare, its surviving row is the minimum row index, its position comes from an ordered scan, and the APD sums are
// sums of ones (exact in int8 up to 127 and in fp32 up to 2^24, whatever the order).
// Invalid molecules get route length 0 and error bits; every index is bounded by the dims, whatever the data holds.
// mix64 and the wave reductions are gi_molread.h's.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int STEP_BITS = 13, STEP_MASK = (1 << STEP_BITS) - 1;     // steps <= 1 + 128 * 127 / 2 = 8129 < 8192
constexpr int SCAN_NT = 1024;
constexpr unsigned EMPTY = 0xFFFFFFFFu;
constexpr u64 EDGE_SALT = 0x9E3779B97F4A7C15ull;

struct Segs { int n; int size[4]; int prod; };

__host__ __device__ __forceinline__ size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }

__global__ __launch_bounds__(64) void route_plan_kernel(const i8* __restrict__ nodes, const i8* __restrict__ edges,
                                                        int N, int Fn, int Fe, Segs sg, u16* __restrict__ estep,
                                                        u16* __restrict__ nstep, u64* __restrict__ nh,
                                                        int* __restrict__ lengths, int* __restrict__ mol_err,
                                                        int* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char smem[];
    u16* tab = (u16*)smem;                                             // [N, N]: type + 1, then step | type << 13
    int* cnt = (int*)(smem + r16((size_t)N * N * 2));                  // [N] steps of node i
    int* start = cnt + N;                                              // [N] first step of node i
    unsigned char* present = (unsigned char*)(start + N);              // [N]
    __shared__ int err_sh, n_sh;
    const int m = blockIdx.x, lane = threadIdx.x;
    const i8* nd = nodes + (size_t)m * N * Fn;
    const i8* ed = edges + (size_t)m * N * N * Fe;
    if (lane == 0) err_sh = 0;
    int err = 0;
    for (int i = lane; i < N; i += 64) {
        const i8* row = nd + i * Fn;
        int any = 0, bad = 0, f = 0;
        u64 h = 0;
        for (int s = 0; s < sg.n; ++s) {
            int sum = 0;
            for (int q = 0; q < sg.size[s]; ++q, ++f) {
                const int v = row[f];
                if (v != 0 && v != 1) err |= GI_ROUTE_ERR_VALUE;
                if (v) { ++sum; h += mix64((u64)(i * Fn + f)); }
            }
            any |= sum;
            bad |= sum != 1;
        }
        if (any && bad) err |= GI_ROUTE_ERR_ONEHOT;
        present[i] = any != 0;
        nh[(size_t)m * N + i] = h;
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0;
        for (int i = 0; i < N; ++i) n += present[i];
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;
    if (n == 0) err |= GI_ROUTE_ERR_EMPTY;
    for (int i = lane; i < N; i += 64)
        if ((present[i] != 0) != (i < n)) err |= GI_ROUTE_ERR_PADDING;
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        const i8* p = ed + (size_t)e * Fe;
        const i8* pt = ed + ((size_t)j * N + i) * Fe;
        int c = 0, t = 0;
        for (int q = 0; q < Fe; ++q) {
            const int v = p[q];
            if (v != 0 && v != 1) err |= GI_ROUTE_ERR_VALUE;
            if (v) { ++c; t = q; }
            if (v != pt[q]) err |= GI_ROUTE_ERR_ASYMMETRIC;
        }
        if (c > 1) err |= GI_ROUTE_ERR_MULTI_BOND;
        if (c && (i == j || i >= n || j >= n)) err |= GI_ROUTE_ERR_PADDING;
        tab[e] = (u16)(c ? t + 1 : 0);
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        int d = 0;
        for (int j = 0; j < i; ++j) d += tab[i * N + j] != 0;
        int c = 0;
        if (i < n) {
            if (i == 0) c = 1;
            else { if (d == 0) err |= GI_ROUTE_ERR_CONNECT; c = d; }
        }
        cnt[i] = c;
    }
    if (err) atomicOr(&err_sh, err);
    __syncthreads();
    if (lane == 0) {
        int run = 1;
        for (int i = N - 1; i >= 0; --i) {
            start[i] = run;
            nstep[(size_t)m * N + i] = (u16)(i < n ? run + cnt[i] - 1 : 0);
            run += cnt[i];
        }
        const int e = err_sh;
        lengths[m] = e ? 0 : run;                         // 1 + sum c_i = n_edges + 2
        mol_err[m] = e;
        if (e) atomicOr(&counts[0], e);
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        if (i == 0 || i >= n) continue;
        int r = 0;
        // descending (type, index); type-0 codes (< 8192, possibly <= Fe) are written in the last sweep, after
        // every comparison against a type + 1 value of this row that could confuse them
        for (int t = Fe - 1; t >= 0; --t)
            for (int j = i - 1; j >= 0; --j)
                if (tab[i * N + j] == t + 1) {
                    const u16 code = (u16)((start[i] + r) | (t << STEP_BITS));
                    ++r;
                    tab[i * N + j] = code;
                    tab[j * N + i] = code;
                }
    }
    __syncthreads();
    u16* out = estep + (size_t)m * N * N;
    for (int e = lane; e < N * N; e += 64) out[e] = tab[e];
}

// Exclusive scan of in[0:n] by one workgroup (the chunked ballot scan of gi_eval.hip): out[i] = sum_{i' < i} in[i'],
// out[n] = the total, also stored to *total; list[out[i]] = i where in[i] != 0 (flags only; may be NULL).
__global__ __launch_bounds__(SCAN_NT) void route_scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out,
                                                             int* __restrict__ total, int* __restrict__ list) {
    constexpr int NW = SCAN_NT / 64;
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int base = 0;
    for (int c = 0; c < n; c += SCAN_NT) {
        const int i = c + tid;
        const int v = i < n ? in[i] : 0;
        int x = v;                                        // inclusive scan inside the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int y = __shfl_up(x, s);
            if (lane >= s) x += y;
        }
        __syncthreads();                                  // the previous chunk's wsum reads are done
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
        int o = base;
        for (int w = 0; w < wid; ++w) o += wsum[w];
        if (i < n) {
            out[i] = o + x - v;
            if (list && v) list[o + x - v] = i;
        }
        for (int w = 0; w < NW; ++w) base += wsum[w];
    }
    if (tid == 0) { out[n] = base; *total = base; }
}

__global__ __launch_bounds__(256) void route_rows_kernel(const i8* __restrict__ nodes, int M, int N, int Fn, int Fe,
                                                         Segs sg, int width, const u16* __restrict__ estep,
                                                         const u16* __restrict__ nstep, const u64* __restrict__ nh,
                                                         const int* __restrict__ off, const int* __restrict__ counts,
                                                         int cap, u64 hash_mask, int* __restrict__ hot,
                                                         u64* __restrict__ hash, int* __restrict__ row_mol,
                                                         int* __restrict__ row_step) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= cap) return;
    const int total = min(counts[1], cap);
    if (r >= total) {
        if (lane == 0) { row_mol[r] = -1; row_step[r] = -1; hot[r] = width - 1; hash[r] = ~0ull; }
        return;
    }
    int lo = 0, hi = M;                                   // the last molecule whose offset is <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    const int m = lo, k = r - off[m];
    const u16* ns = nstep + (size_t)m * N;
    const u16* es = estep + (size_t)m * N * N;
    u64 h = 0;
    int ci = -1;                                          // the node step k works on: the last one still there before it
    for (int i = lane; i < N; i += 64) {
        const int s = ns[i];
        if (s > k) h += nh[(size_t)m * N + i];
        if (s >= k && s > 0) ci = max(ci, i);
    }
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        const int code = es[e];
        if (j < i && (code & STEP_MASK) > k) h += mix64(EDGE_SALT + (u64)e * Fe + (code >> STEP_BITS));
    }
    h = wave_sum64(h) & hash_mask;
    ci = wave_max(ci);
    int hot_idx = width - 1;                              // k = 0: terminate
    if (k > 0 && ci >= 0) {
        int found = -1;
        for (int j = lane; j < ci; j += 64) {
            const int code = es[ci * N + j];
            if ((code & STEP_MASK) == k) found = (j << 3) | (code >> STEP_BITS);
        }
        found = wave_max(found);
        const int j = found < 0 ? 0 : found >> 3, t = found < 0 ? 0 : found & 7;
        if (k == ns[ci]) {                                // the node's last bond: f_add[j, features.., t]
            const i8* row = nodes + ((size_t)m * N + ci) * Fn;
            int idx = 0, f = 0;
            for (int s = 0; s < sg.n; ++s) {
                int pos = 0;
                for (int q = 0; q < sg.size[s]; ++q, ++f)
                    if (row[f]) pos = q;
                idx = idx * sg.size[s] + pos;
            }
            hot_idx = (j * sg.prod + idx) * Fe + t;
        } else {
            hot_idx = N * sg.prod * Fe + j * Fe + t;
        }
    }
    if (lane == 0) { row_mol[r] = m; row_step[r] = k; hot[r] = hot_idx; hash[r] = h; }
}

// pieces [0, pn) cover out_nodes, [pn, pn + pe) out_edges, [pn + pe, pn + pe + pa) out_apd, 16 bytes each; the
// buffers are padded to whole pieces by the caller.  Rows past the real total come out zero.
template <int APD>                                        // 0 none, 1 int8, 2 fp32
__global__ __launch_bounds__(256) void route_expand_kernel(const i8* __restrict__ nodes, int N, int Fn, int Fe,
                                                           int width, const u16* __restrict__ estep,
                                                           const u16* __restrict__ nstep,
                                                           const int* __restrict__ row_mol,
                                                           const int* __restrict__ row_step,
                                                           const int* __restrict__ hot,
                                                           const int* __restrict__ counts, int cap,
                                                           i8* __restrict__ out_nodes, i8* __restrict__ out_edges,
                                                           void* __restrict__ out_apd, long long pn, long long pe,
                                                           long long pa) {
    long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int total = min(counts[1], cap);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (p < pn) {
        const int pitch = N * Fn;
        const long long b0 = p * 16;
        int row = (int)(b0 / pitch), o = (int)(b0 - (long long)row * pitch);
        int i = o / Fn, f = o - i * Fn;
        int m = 0, k = 0;
        bool live = row < total, alive = false;
        if (live) { m = row_mol[row]; k = row_step[row]; alive = nstep[(size_t)m * N + i] > k; }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (live && alive) w[q >> 2] |= (unsigned)(nodes[(size_t)m * pitch + o] & 0xff) << ((q & 3) * 8);
            ++o;
            if (++f == Fn) {
                f = 0; ++i;
                if (o == pitch) {
                    o = 0; i = 0; ++row;
                    live = row < total;
                    if (live) { m = row_mol[row]; k = row_step[row]; }
                }
                alive = live && nstep[(size_t)m * N + i] > k;
            }
        }
        *reinterpret_cast<uint4*>(out_nodes + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    p -= pn;
    if (p < pe) {
        const int NN = N * N, pitch = NN * Fe;
        const long long b0 = p * 16;
        int row = (int)(b0 / pitch), o = (int)(b0 - (long long)row * pitch);
        int e = o / Fe, t = o - e * Fe;
        int m = 0, k = 0, code = 0;
        bool live = row < total;
        if (live) { m = row_mol[row]; k = row_step[row]; code = estep[(size_t)m * NN + e]; }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (live && (code & STEP_MASK) > k && (code >> STEP_BITS) == t) w[q >> 2] |= 1u << ((q & 3) * 8);
            if (++t == Fe) {
                t = 0;
                if (++e == NN) {
                    e = 0; ++row;
                    live = row < total;
                    if (live) { m = row_mol[row]; k = row_step[row]; }
                }
                code = live ? estep[(size_t)m * NN + e] : 0;
            }
        }
        *reinterpret_cast<uint4*>(out_edges + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    p -= pe;
    if (APD == 0 || p >= pa) return;
    if (APD == 1) {
        const long long b0 = p * 16;
        int row = (int)(b0 / width), o = (int)(b0 - (long long)row * width);
        int hr = row < total ? hot[row] : -1;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (o == hr) w[q >> 2] |= 1u << ((q & 3) * 8);
            if (++o == width) { o = 0; ++row; hr = row < total ? hot[row] : -1; }
        }
        *reinterpret_cast<uint4*>((i8*)out_apd + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const long long e0 = p * 4;
        int row = (int)(e0 / width), o = (int)(e0 - (long long)row * width);
        int hr = row < total ? hot[row] : -1;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = o == hr ? 1.f : 0.f;
            if (++o == width) { o = 0; ++row; hr = row < total ? hot[row] : -1; }
        }
        *reinterpret_cast<float4*>((float*)out_apd + e0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// One wave per row: walk the table from the row's hash; an empty slot is claimed, a slot whose owner row has the same
// bytes is joined, any other is passed.  Rows of one graph share a hash, hence a probe sequence, and slots are never
// released, so they all end in one slot, whichever of them claimed it.
__global__ __launch_bounds__(256) void route_insert_kernel(const i8* __restrict__ rn, int pitch_n,
                                                           const i8* __restrict__ re, int pitch_e,
                                                           const u64* __restrict__ hash,
                                                           const int* __restrict__ counts, int cap,
                                                           unsigned* __restrict__ slot, unsigned* __restrict__ minrow,
                                                           unsigned tmask, int* __restrict__ slot_of) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int total = min(counts[1], cap);
    if (r >= total) return;
    unsigned s = (unsigned)hash[r] & tmask;
    for (unsigned it = 0; it <= tmask; ++it, s = (s + 1) & tmask) {
        unsigned v = 0;
        if (lane == 0) v = atomicCAS(&slot[s], EMPTY, (unsigned)r);
        v = (unsigned)__shfl((int)v, 0);
        if (v == EMPTY || v == (unsigned)r) break;
        if (v >= (unsigned)total) continue;               // cannot happen: only rows < total are inserted
        bool diff = false;
        const i8* a = rn + (size_t)r * pitch_n;
        const i8* b = rn + (size_t)v * pitch_n;
        for (int q = lane; q < pitch_n; q += 64) diff |= a[q] != b[q];
        a = re + (size_t)r * pitch_e;
        b = re + (size_t)v * pitch_e;
        for (int q = lane; q < pitch_e; q += 64) diff |= a[q] != b[q];
        if (!__any(diff)) break;
    }
    if (lane == 0) { slot_of[r] = (int)s; atomicMin(&minrow[s], (unsigned)r); }
}

// rep[r] = the first row of r's class (overwrites slot_of), keep[r] = r is that row
__global__ __launch_bounds__(256) void route_rep_kernel(int* __restrict__ slot_of, const unsigned* __restrict__ minrow,
                                                        const int* __restrict__ counts, int cap,
                                                        int* __restrict__ keep) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= cap) return;
    const int total = min(counts[1], cap);
    if (r >= total) { keep[r] = 0; return; }
    const int rep = (int)minrow[slot_of[r]];
    slot_of[r] = rep;
    keep[r] = rep == r;
}

__global__ __launch_bounds__(256) void route_gather_kernel(const i8* __restrict__ rn, int pitch_n,
                                                           const i8* __restrict__ re, int pitch_e,
                                                           const int* __restrict__ kept,
                                                           const int* __restrict__ counts,
                                                           i8* __restrict__ out_nodes, i8* __restrict__ out_edges,
                                                           long long pn, long long pe) {
    long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int mtotal = counts[2];
    const i8* src = rn;
    i8* dst = out_nodes;
    int pitch = pitch_n;
    if (p >= pn) { p -= pn; src = re; dst = out_edges; pitch = pitch_e; if (p >= pe) return; }
    const long long b0 = p * 16;
    int row = (int)(b0 / pitch), o = (int)(b0 - (long long)row * pitch);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    const i8* s = row < mtotal ? src + (size_t)kept[row] * pitch : nullptr;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (s) w[q >> 2] |= (unsigned)(s[o] & 0xff) << ((q & 3) * 8);
        if (++o == pitch) { o = 0; ++row; s = row < mtotal ? src + (size_t)kept[row] * pitch : nullptr; }
    }
    *reinterpret_cast<uint4*>(dst + b0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// out_apd[newpos[rep[r]], hot[r]] += 1 (int8: an add on the enclosing aligned word; a byte never exceeds 127 because
// a class has at most one row per molecule and int8 is used for M <= 127 only); (molecule, step) of the kept rows
template <bool F32>
__global__ __launch_bounds__(256) void route_apd_kernel(const int* __restrict__ rep, const int* __restrict__ keep,
                                                        const int* __restrict__ newpos, const int* __restrict__ hot,
                                                        const int* __restrict__ row_mol,
                                                        const int* __restrict__ row_step,
                                                        const int* __restrict__ counts, int cap, int width,
                                                        void* __restrict__ out_apd, int* __restrict__ out_mol,
                                                        int* __restrict__ out_step) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int total = min(counts[1], cap);
    if (r >= total) return;
    const int d = newpos[rep[r]];
    const size_t at = (size_t)d * width + hot[r];
    if (F32) atomicAdd((float*)out_apd + at, 1.f);
    else atomicAdd((unsigned*)out_apd + (at >> 2), 1u << ((at & 3) * 8));
    if (keep[r]) { out_mol[d] = row_mol[r]; out_step[d] = row_step[r]; }
}

struct PlanWs { size_t estep, nstep, nh, off, total; };
struct RowsWs { size_t hot, hash, slot, minrow, slot_of, keep, newpos, kept, total; unsigned tsize; };

int check_dims(const gi_route_dims* d, Segs* sg) {
    if (!d || d->M < 0 || d->N < 1 || d->Fn < 1 || d->Fe < 1 || d->n_seg < 1 || d->n_seg > 4) return GI_EINVAL;
    if (d->N > GI_MAX_NODES || d->Fe > GI_MAX_GROUPS) return GI_ELIMIT;
    long long sum = 0, prod = 1;
    sg->n = d->n_seg;
    for (int s = 0; s < 4; ++s) {
        sg->size[s] = s < d->n_seg ? d->seg[s] : 0;
        if (s < d->n_seg) {
            if (d->seg[s] < 1) return GI_EINVAL;
            sum += d->seg[s];
            prod *= d->seg[s];
            if (prod > (1 << 24)) return GI_ELIMIT;
        }
    }
    const long long width = (long long)d->N * prod * d->Fe + (long long)d->N * d->Fe + 1;
    if (sum != d->Fn || width != d->apd_width) return GI_EINVAL;
    if (width > 0x7fffffffLL) return GI_ELIMIT;
    sg->prod = (int)prod;
    return 0;
}

PlanWs plan_layout(const gi_route_dims* d) {
    PlanWs w;
    size_t o = 0;
    const size_t M = (size_t)d->M, N = (size_t)d->N;
    w.estep = o; o += r16(M * N * N * 2);
    w.nstep = o; o += r16(M * N * 2);
    w.nh = o; o += r16(M * N * 8);
    w.off = o; o += r16((M + 1) * 4);
    w.total = o;
    return w;
}

RowsWs rows_layout(int cap, int merge) {
    RowsWs w;
    size_t o = 0;
    const size_t R = (size_t)cap;
    unsigned T = 64;
    while ((size_t)T < 2 * R) T <<= 1;
    w.tsize = T;
    w.hot = o; o += r16(R * 4);
    w.hash = o; o += r16(R * 8);
    w.slot = w.minrow = w.slot_of = w.keep = w.newpos = w.kept = o;
    if (merge) {
        w.slot = o; o += r16((size_t)T * 4);
        w.minrow = o; o += r16((size_t)T * 4);             // directly behind slot: one memset sets both
        w.slot_of = o; o += r16(R * 4);
        w.keep = o; o += r16(R * 4);
        w.newpos = o; o += r16((R + 1) * 4);
        w.kept = o; o += r16(R * 4);
    }
    w.total = o;
    return w;
}

constexpr int MAX_ROWS = 1 << 29;                         // 2 * rows must fit the 32-bit table index

}  // namespace

extern "C" long long gi_route_plan_ws_bytes(const gi_route_dims* d) {
    Segs sg;
    const int rc = check_dims(d, &sg);
    if (rc) return rc;
    return (long long)plan_layout(d).total;
}

extern "C" long long gi_route_rows_ws_bytes(int rows_cap, int merge) {
    if (rows_cap < 0) return GI_EINVAL;
    if (rows_cap > MAX_ROWS) return GI_ELIMIT;
    return (long long)rows_layout(rows_cap, merge).total;
}

extern "C" int gi_route_rows_hot(void* rows_ws, int rows_cap, int** hot) {
    if (!rows_ws || !hot || rows_cap < 0) return GI_EINVAL;
    if (rows_cap > MAX_ROWS) return GI_ELIMIT;
    *hot = (int*)((char*)rows_ws + rows_layout(rows_cap, 0).hot);
    return 0;
}

extern "C" int gi_route_plan(const gi_route_dims* d, const signed char* nodes, const signed char* edges,
                             void* plan_ws, int* lengths, int* mol_err, int* counts, void* stream) {
    (void)hipGetLastError();
    Segs sg;
    const int rc = check_dims(d, &sg);
    if (rc) return rc;
    if (!counts) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, GI_ROUTE_COUNTS * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (d->M == 0) return 0;
    if (!nodes || !edges || !plan_ws || !lengths || !mol_err) return GI_EINVAL;
    const PlanWs w = plan_layout(d);
    char* ws = (char*)plan_ws;
    const int N = d->N;
    const size_t lds = r16((size_t)N * N * 2) + (size_t)N * 8 + r16((size_t)N);
    hipLaunchKernelGGL(route_plan_kernel, dim3(d->M), dim3(64), lds, st, nodes, edges, N, d->Fn, d->Fe, sg,
                       (u16*)(ws + w.estep), (u16*)(ws + w.nstep), (u64*)(ws + w.nh), lengths, mol_err, counts);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, (const int*)lengths, d->M,
                       (int*)(ws + w.off), counts + 1, (int*)nullptr);
    return gi_launch_status();
}

extern "C" int gi_route_expand(const gi_route_dims* d, const signed char* nodes, const void* plan_ws, void* rows_ws,
                               const int* counts, int rows_cap, unsigned long long hash_mask,
                               signed char* out_nodes, signed char* out_edges, void* out_apd, int apd_dtype,
                               int* row_mol, int* row_step, void* stream) {
    (void)hipGetLastError();
    Segs sg;
    const int rc = check_dims(d, &sg);
    if (rc) return rc;
    if (rows_cap < 0) return GI_EINVAL;
    if (rows_cap > MAX_ROWS) return GI_ELIMIT;
    if (rows_cap == 0 || d->M == 0) return 0;
    if (!nodes || !plan_ws || !rows_ws || !counts || !out_nodes || !out_edges || !row_mol || !row_step)
        return GI_EINVAL;
    if (out_apd && apd_dtype != GI_DTYPE_F32 && apd_dtype != GI_DTYPE_I8) return GI_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const PlanWs pw = plan_layout(d);
    const RowsWs rw = rows_layout(rows_cap, 0);           // hot and hash sit in front, whatever `merge` was
    const char* pws = (const char*)plan_ws;
    char* rws = (char*)rows_ws;
    const u16* estep = (const u16*)(pws + pw.estep);
    const u16* nstep = (const u16*)(pws + pw.nstep);
    int* hot = (int*)(rws + rw.hot);
    const int N = d->N, Fn = d->Fn, Fe = d->Fe, W = d->apd_width;
    hipLaunchKernelGGL(route_rows_kernel, dim3(gi_cdiv(rows_cap, 4)), dim3(256), 0, st, nodes, d->M, N, Fn, Fe, sg, W,
                       estep, nstep, (const u64*)(pws + pw.nh), (const int*)(pws + pw.off), counts, rows_cap,
                       (u64)hash_mask, hot, (u64*)(rws + rw.hash), row_mol, row_step);
    const long long R = rows_cap;
    const long long pn = (R * N * Fn + 15) / 16, pe = (R * N * N * Fe + 15) / 16;
    const long long pa = !out_apd ? 0 : apd_dtype == GI_DTYPE_I8 ? (R * W + 15) / 16 : (R * W + 3) / 4;
    const long long blocks = (pn + pe + pa + 255) / 256;
    if (blocks > 0x7fffffffLL) return GI_ELIMIT;
#define GI_ROUTE_EXPAND(A_)                                                                                   \
    hipLaunchKernelGGL((route_expand_kernel<A_>), dim3((unsigned)blocks), dim3(256), 0, st, nodes, N, Fn, Fe, W, \
                       estep, nstep, (const int*)row_mol, (const int*)row_step, (const int*)hot, counts,      \
                       rows_cap, out_nodes, out_edges, out_apd, pn, pe, pa)
    if (!out_apd) GI_ROUTE_EXPAND(0);
    else if (apd_dtype == GI_DTYPE_I8) GI_ROUTE_EXPAND(1);
    else GI_ROUTE_EXPAND(2);
#undef GI_ROUTE_EXPAND
    return gi_launch_status();
}

extern "C" int gi_route_merge(const gi_route_dims* d, void* rows_ws, int* counts, int rows_cap,
                              const signed char* in_nodes, const signed char* in_edges, const int* in_row_mol,
                              const int* in_row_step, signed char* out_nodes, signed char* out_edges, void* out_apd,
                              int apd_dtype, int* out_row_mol, int* out_row_step, void* stream) {
    (void)hipGetLastError();
    Segs sg;
    const int rc = check_dims(d, &sg);
    if (rc) return rc;
    if (rows_cap < 0) return GI_EINVAL;
    if (rows_cap > MAX_ROWS) return GI_ELIMIT;
    if (rows_cap == 0 || d->M == 0) return 0;
    if (!rows_ws || !counts || !in_nodes || !in_edges || !in_row_mol || !in_row_step || !out_nodes || !out_edges ||
        !out_apd || !out_row_mol || !out_row_step)
        return GI_EINVAL;
    if (apd_dtype != GI_DTYPE_F32 && apd_dtype != GI_DTYPE_I8) return GI_EINVAL;
    if (apd_dtype == GI_DTYPE_I8 && d->M > 127) return GI_EINVAL;      // a sum may reach M
    const hipStream_t st = (hipStream_t)stream;
    const RowsWs rw = rows_layout(rows_cap, 1);
    char* ws = (char*)rows_ws;
    unsigned* slot = (unsigned*)(ws + rw.slot);
    unsigned* minrow = (unsigned*)(ws + rw.minrow);
    int* slot_of = (int*)(ws + rw.slot_of);
    int* keep = (int*)(ws + rw.keep);
    int* newpos = (int*)(ws + rw.newpos);
    int* kept = (int*)(ws + rw.kept);
    const int* hot = (const int*)(ws + rw.hot);
    const int pitch_n = d->N * d->Fn, pitch_e = d->N * d->N * d->Fe, W = d->apd_width;
    const long long R = rows_cap;
    const size_t apd_bytes = apd_dtype == GI_DTYPE_I8 ? (size_t)((R * W + 15) / 16 * 16) : (size_t)(R * W) * 4;
    hipError_t e = hipMemsetAsync(slot, 0xFF, rw.slot_of - rw.slot, st);       // slot and minrow
    if (e == hipSuccess) e = hipMemsetAsync(out_apd, 0, apd_bytes, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(route_insert_kernel, dim3(gi_cdiv(rows_cap, 4)), dim3(256), 0, st, in_nodes, pitch_n, in_edges,
                       pitch_e, (const u64*)(ws + rw.hash), (const int*)counts, rows_cap, slot, minrow,
                       rw.tsize - 1, slot_of);
    hipLaunchKernelGGL(route_rep_kernel, dim3(gi_cdiv(rows_cap, 256)), dim3(256), 0, st, slot_of,
                       (const unsigned*)minrow, (const int*)counts, rows_cap, keep);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, (const int*)keep, rows_cap, newpos,
                       counts + 2, kept);
    const long long pn = (R * pitch_n + 15) / 16, pe = (R * pitch_e + 15) / 16;
    const long long blocks = (pn + pe + 255) / 256;
    if (blocks > 0x7fffffffLL) return GI_ELIMIT;
    hipLaunchKernelGGL(route_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in_nodes, pitch_n, in_edges,
                       pitch_e, (const int*)kept, (const int*)counts, out_nodes, out_edges, pn, pe);
#define GI_ROUTE_APD(F_)                                                                                       \
    hipLaunchKernelGGL((route_apd_kernel<F_>), dim3(gi_cdiv(rows_cap, 256)), dim3(256), 0, st, (const int*)slot_of, \
                       (const int*)keep, (const int*)newpos, hot, in_row_mol, in_row_step, (const int*)counts,  \
                       rows_cap, W, out_apd, out_row_mol, out_row_step)
    if (apd_dtype == GI_DTYPE_F32) GI_ROUTE_APD(true); else GI_ROUTE_APD(false);
#undef GI_ROUTE_APD
    return gi_launch_status();
}
