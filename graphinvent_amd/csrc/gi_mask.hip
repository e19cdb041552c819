// The action mask of constrained generation on the device (gfx950): between the forward and the draw of a generation
// round, every action the growth step would reject (attach to a slot without an atom, bond a bonded pair, add to a full
// graph) or that would take an atom over its valence is set to -inf in a COPY of the logits, so that the unmodified
// sampler (gi_sample.hip: osm_add skips -inf, only e > 0 is drawn) draws from the renormalised distribution.  The rule
// is written out at gi_action_mask in the public header; tests/action_mask_model.py is its numpy specification.
// THE VALENCE TABLE IS THE CALLER'S (analyze.ValenceRules), NOT RDKit's.
//
// action_mask_kernel  one 256-lane WORKGROUP per graph:
//   1  gi_read_labelled of gi_molread.h (the front end of gi_valence.hip, gi_fingerprint.hip, gi_smiles.hip): the
//      state is read once in 16-byte granules (fp32 or int8) into 128-bit adjacency rows in LDS, the structure bits
//      set while reading; the lane of atom i leaves with twice its bond-order sum and the OR of its rows;
//   2  tables in LDS: lane i < N: budget2(i), then the two per-node thresholds addb[i] / conb[i] (the structural rules
//      folded in as "nothing fits"); lane k < T C H: lim2[k] = 2 vmax - 2 h of a (type, charge, h) combination;
//   3  all lanes stride over the row in items of 4 columns.  An add column is decoded by a mixed-radix counter
//      (node, combination, rest, bond type) that is advanced by the item stride with carries: the strides are divided
//      out once, in front of the loop, and the loop itself divides only in the connect block (one division per
//      column).  admissible = order2[f] <= addb[i] && order2[f] <= lim2[k] (add), order2[f] <= conb[i] (connect).
//      For up to two logits matrices the item is loaded (16 bytes where base and pitch allow, else by element),
//      inadmissible columns become -inf, and it is stored the same way; the bits of 8 lanes make one word of the
//      packed mask; an online softmax of the first matrix gives the probability mass the mask removes.
// Integers decide everything but that last figure.  No global atomics, no scratch, no memset, nothing read back.
// Every index is bounded by the dims (see gi_read_labelled; i < N, k < T C H by the counter's carries, f < Fe).
// LDS: Fe N 16 B dynamic (<= 16 KB), ~14 KB static.
#include <climits>

#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int COLS = 4;                                      // columns of an item: one 16-byte access
constexpr unsigned NEG_INF = 0xff800000u;
constexpr int NOTHING = INT_MIN, ANYTHING = 127;             // thresholds no / every order2 passes

struct MaskRules {
    const unsigned short* allowed;                           // [T * C]: bit v = total valence v is allowed
    const i8* order2;                                        // [Fe] twice the bond order
    const i8* h_values;                                      // [H] the stored implicit-H counts (H > 0)
    int T, C, H;
    int rest;                                                // product of the node-feature groups behind the segments
    int combos;                                              // T * C * max(H, 1)
    int valence, allow_empty;
};

struct MaskRows {                                            // up to two logits matrices and their masked copies
    const unsigned* in[2];
    unsigned* out[2];
    int ldi[2], ldo[2], vin[2], vout[2];                     // row pitches; 16-byte access allowed
};

struct MaskOut {
    int* n_admissible;
    int* status;
    unsigned* bits;                                          // [B][words] or nullptr
    float* removed;                                          // [B] or nullptr
    int words;
};

struct AddColumn {                                           // an add column as (node, combination, rest, bond type)
    int i, k, r, f;
};

__device__ __forceinline__ int top_valence2(unsigned mask) { return mask ? 2 * (31 - __clz((int)mask)) : -2; }

template <typename T>
__global__ __launch_bounds__(NT) void action_mask_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                         const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                         int Fe, int A, int W, MaskRules rl, MaskRows rows, MaskOut out) {
    extern __shared__ unsigned adj[];                        // [Fe][N][4]: bit j of row (t, i): bond t between i and j
    __shared__ GiLabelled st;
    __shared__ int bud2[MAXN], addb[MAXN], conb[MAXN];
    __shared__ short lim2[GI_MASK_MAX_COMBOS];
    __shared__ int wcnt[NT / 64];
    __shared__ float wmax[NT / 64], wall[NT / 64], wkept[NT / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;

    // ---- 1: read and check -----------------------------------------------------------------------------------
    GiLabelledNode me;
    const int n = gi_read_labelled<true>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes,
                                         nn_bytes, g, N, Fn, Fe, rl.T, rl.C, rl.H, rl.order2, tid, adj, st, nullptr, me);
    const int ill = st.flags & (GI_MOL_MALFORMED | GI_LABEL_SELF_LOOP);                  // uniform
    const bool val = ill == 0 && rl.valence != 0;            // the valence rules apply

    // ---- 2: the tables -----------------------------------------------------------------------------------------
    if (tid < N) {
        int b2 = 0;
        if (val && tid < n) {                                // the row is one-hot: a < T, c < C, the H index < H
            const int a = st.seg_first[0][tid], c = st.seg_first[1][tid];
            const int s = rl.H > 0 ? (int)rl.h_values[st.seg_first[2][tid]] : 0;
            b2 = top_valence2((unsigned)rl.allowed[a * rl.C + c]) - me.o2 - 2 * s;
        }
        bud2[tid] = b2;
    }
    for (int k = tid; k < rl.combos; k += NT) {
        int v = ANYTHING;
        if (val) {
            const int tc = rl.H > 0 ? k / rl.H : k;
            const int h = rl.H > 0 ? (int)rl.h_values[k - tc * rl.H] : 0;
            v = top_valence2((unsigned)rl.allowed[tc]) - 2 * h;
        }
        lim2[k] = (short)v;                                  // >= -2 - 254
    }
    __syncthreads();
    if (tid < N) {
        const bool add_ok = n < N && (n == 0 ? tid == 0 : tid < n);
        addb[tid] = !add_ok ? NOTHING : (val && n >= 1) ? bud2[tid] : ANYTHING;
        const int lw = (n - 1) >> 5;                         // (selected, not indexed: me.seen stays in registers)
        const unsigned last = lw == 0 ? me.seen[0] : lw == 1 ? me.seen[1] : lw == 2 ? me.seen[2] : me.seen[3];
        const bool con_ok = n >= 2 && tid < n - 1 && !((last >> ((n - 1) & 31)) & 1u);
        conb[tid] = !con_ok ? NOTHING : val ? min(bud2[tid], bud2[n - 1]) : ANYTHING;
    }
    __syncthreads();
    unsigned long long o2pack = 0ull;                        // order2[f] in byte f; the empty graph's add sets no bond
    if (n > 0)
        for (int f = 0; f < Fe; ++f) o2pack |= (unsigned long long)(unsigned char)rl.order2[f] << (8 * f);
    const bool term_ok = n >= 1 || rl.allow_empty != 0;

    // ---- 3: the rows -------------------------------------------------------------------------------------------
    const int NA = N * A, items = (W + COLS - 1) / COLS;
    const int rest = rl.rest, combos = rl.combos;
    auto split = [&](int j, AddColumn& c) {                  // column j of the add block; also: a stride of j columns
        c.i = j / A;
        const int rem = j - c.i * A, q = rem / Fe;
        c.f = rem - q * Fe;
        c.k = q / rest;
        c.r = q - c.k * rest;
    };
    auto advance = [&](AddColumn& c, const AddColumn& d) {   // c += d with carries: every digit stays below its radix
        c.f += d.f;
        int carry = c.f >= Fe;
        c.f -= carry ? Fe : 0;
        c.r += d.r + carry;
        carry = c.r >= rest;
        c.r -= carry ? rest : 0;
        c.k += d.k + carry;
        carry = c.k >= combos;
        c.k -= carry ? combos : 0;
        c.i += d.i + carry;
    };
    AddColumn stride, base;
    const AddColumn one = {0, 0, 0, 1};
    split(COLS * NT, stride);                                // uniform: hoisted out of the loop
    split(COLS * tid, base);                                 // once per lane (past the add block: never looked at)
    const bool stats = out.removed != nullptr;
    int cnt = 0;
    float mx = -INFINITY, s_all = 0.f, s_kept = 0.f;
    for (int k0 = 0; k0 < items; k0 += NT) {                 // uniform trip count: the shuffles below see every lane
        const int item = k0 + tid, j0 = COLS * item;
        unsigned nib = 0u;
        if (item < items) {
            AddColumn c = base;
#pragma unroll
            for (int e = 0; e < COLS; ++e) {
                const int j = j0 + e;
                bool ok = false;
                if (j < NA) {                                // c.i < N, c.k < combos, c.f < Fe
                    const int o2 = (int)((o2pack >> (8 * c.f)) & 0xffull);
                    ok = o2 <= addb[c.i] && o2 <= (int)lim2[c.k];
                    advance(c, one);
                } else if (j < W - 1) {
                    const int q = j - NA, i = q / Fe;        // i < N
                    ok = (int)((o2pack >> (8 * (q - i * Fe))) & 0xffull) <= conb[i];
                } else if (j == W - 1) {
                    ok = term_ok;
                }
                nib |= (ok ? 1u : 0u) << e;
            }
            cnt += __popc(nib);
            const bool whole = j0 + COLS <= W;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!rows.in[s]) continue;                   // uniform
                const unsigned* src = rows.in[s] + (size_t)g * rows.ldi[s] + j0;
                unsigned* dst = rows.out[s] + (size_t)g * rows.ldo[s] + j0;
                unsigned v[COLS];
                if (whole && rows.vin[s]) {
                    const uint4 q = *reinterpret_cast<const uint4*>(src);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
#pragma unroll
                    for (int e = 0; e < COLS; ++e) v[e] = j0 + e < W ? src[e] : NEG_INF;
                }
                if (s == 0 && stats) {                       // online softmax: all columns, and the admissible ones
#pragma unroll
                    for (int e = 0; e < COLS; ++e) {
                        const float x = __uint_as_float(v[e]);
                        if (x == -INFINITY) continue;        // (and every column past W)
                        if (x > mx) {
                            const float sc = __expf(mx - x);
                            s_all *= sc;
                            s_kept *= sc;
                            mx = x;
                        }
                        const float ex = __expf(x - mx);
                        s_all += ex;
                        if ((nib >> e) & 1u) s_kept += ex;
                    }
                }
#pragma unroll
                for (int e = 0; e < COLS; ++e)
                    if (!((nib >> e) & 1u)) v[e] = NEG_INF;
                if (whole && rows.vout[s]) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < COLS; ++e)
                        if (j0 + e < W) dst[e] = v[e];
                }
            }
        }
        if (out.bits) {                                      // uniform; 8 lanes x 4 bits = one word
            unsigned w = nib << (COLS * (tid & 7));
            w |= (unsigned)__shfl_xor((int)w, 1);
            w |= (unsigned)__shfl_xor((int)w, 2);
            w |= (unsigned)__shfl_xor((int)w, 4);
            if ((tid & 7) == 0 && j0 < W) out.bits[(size_t)g * out.words + (item >> 3)] = w;   // item >> 3 < words
        }
        advance(base, stride);
    }

    // ---- 4: the per-graph outputs --------------------------------------------------------------------------------
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (stats) {
        float m = mx;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
        const float sc = mx == -INFINITY ? 0.f : __expf(mx - m);
        s_all *= sc;
        s_kept *= sc;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            s_all += __shfl_xor(s_all, s);
            s_kept += __shfl_xor(s_kept, s);
        }
        if ((tid & 63) == 0) { wmax[tid >> 6] = m; wall[tid >> 6] = s_all; wkept[tid >> 6] = s_kept; }
    }
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < NT / 64; ++w) total += wcnt[w];
        out.n_admissible[g] = total;
        out.status[g] = ill | (ill ? GI_MASK_STRUCTURAL : 0);
        if (stats) {
            float m = wmax[0];
            for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, wmax[w]);
            float all = 0.f, kept = 0.f;
            for (int w = 0; w < NT / 64; ++w) {
                const float sc = wmax[w] == -INFINITY ? 0.f : __expf(wmax[w] - m);
                all += wall[w] * sc;
                kept += wkept[w] * sc;
            }
            out.removed[g] = all > 0.f ? fmaxf(1.f - kept / all, 0.f) : 0.f;
        }
    }
}

// acc_i[0] += 1, acc_i[1] += #{removed > 0}, acc_f[0] += sum removed, unless the growth state is frozen; one workgroup,
// a fixed order of additions
__global__ __launch_bounds__(NT) void mask_stats_kernel(int B, const float* __restrict__ removed,
                                                        const int* __restrict__ grow_state, int* acc_i, float* acc_f) {
    __shared__ float sum[NT];
    __shared__ int hit[NT];
    const int tid = threadIdx.x;
    if (grow_state && (grow_state[0] >= grow_state[2] || grow_state[3] != 0)) return;    // uniform: a frozen round
    float s = 0.f;
    int h = 0;
    for (int b = tid; b < B; b += NT) {
        const float r = removed[b];
        if (r > 0.f) { s += r; ++h; }
    }
    sum[tid] = s;
    hit[tid] = h;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) { sum[tid] += sum[tid + o]; hit[tid] += hit[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        acc_i[0] += 1;
        acc_i[1] += hit[0];
        acc_f[0] += sum[0];
    }
}

}  // namespace

extern "C" int gi_action_mask(int B, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                              const void* n_nodes, int n_nodes_bytes, int n_groups, const int* group, int n_types,
                              int n_charges, int n_imp_h, const unsigned short* allowed, const signed char* order2,
                              const signed char* h_values, int valence, int allow_empty, const float* logits, int ldl,
                              float* masked, int ldm, const float* logits2, int ldl2, float* masked2, int ldm2,
                              int* n_admissible, int* status, unsigned* bits, float* removed, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(B, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if ((valence != 0 && valence != 1) || (allow_empty != 0 && allow_empty != 1)) return GI_EINVAL;
    const int n_seg = n_imp_h > 0 ? 3 : 2;
    if (!group || n_groups < n_seg || n_groups > GI_GROW_MAX_GROUPS) return GI_EINVAL;
    long long sum = 0, rest = 1, A = Fe;                     // the add block of one node: prod(group) * Fe columns
    for (int k = 0; k < n_groups; ++k) {
        if (group[k] < 1) return GI_EINVAL;
        sum += group[k];
        if (sum > Fn) return GI_EINVAL;                      // (so every factor is <= Fn <= 512: no overflow below)
        A *= group[k];
        if (k >= n_seg) rest *= group[k];
        if (A > INT_MAX) return GI_ELIMIT;
    }
    if (sum != Fn || group[0] != n_types || group[1] != n_charges || (n_imp_h > 0 && group[2] != n_imp_h))
        return GI_EINVAL;
    const long long W = (long long)N * A + (long long)N * Fe + 1;
    const long long combos = (long long)n_types * n_charges * (n_imp_h > 0 ? n_imp_h : 1);
    if (W > INT_MAX - 4 * GI_MOL_NT || combos > GI_MASK_MAX_COMBOS) return GI_ELIMIT;
    if (ldl < W || ldm < W || (logits2 && (ldl2 < W || ldm2 < W))) return GI_EINVAL;
    if (B == 0) return 0;
    if (!nodes || !edges || !n_nodes || !allowed || !order2 || (n_imp_h > 0 && !h_values) || !logits || !masked ||
        !n_admissible || !status || (logits2 == nullptr) != (masked2 == nullptr))
        return GI_EINVAL;
    if ((const float*)masked == logits || (logits2 && ((const float*)masked2 == logits2 || masked2 == masked)))
        return GI_EINVAL;                                    // a masked copy is never the matrix it is made from
    const MaskRules rl = {allowed, order2, h_values, n_types, n_charges, n_imp_h, (int)rest, (int)combos, valence,
                          allow_empty};
    auto wide = [](const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && (ld & 3) == 0 ? 1 : 0; };
    MaskRows rows = {};
    rows.in[0] = (const unsigned*)logits;
    rows.out[0] = (unsigned*)masked;
    rows.ldi[0] = ldl;
    rows.ldo[0] = ldm;
    rows.vin[0] = wide(logits, ldl);
    rows.vout[0] = wide(masked, ldm);
    if (logits2) {
        rows.in[1] = (const unsigned*)logits2;
        rows.out[1] = (unsigned*)masked2;
        rows.ldi[1] = ldl2;
        rows.ldo[1] = ldm2;
        rows.vin[1] = wide(logits2, ldl2);
        rows.vout[1] = wide(masked2, ldm2);
    }
    const MaskOut out = {n_admissible, status, bits, removed, (int)((W + 31) / 32)};
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned);                                      // <= 16 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(action_mask_kernel<float>, dim3(B), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, (int)A, (int)W, rl, rows, out);
    else
        hipLaunchKernelGGL(action_mask_kernel<i8>, dim3(B), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, (int)A, (int)W, rl, rows, out);
    return gi_launch_status();
}

extern "C" int gi_action_mask_stats(int B, const float* removed, const int* grow_state, int* acc_counts,
                                    float* acc_mass, void* stream) {
    (void)hipGetLastError();
    if (B < 0) return GI_EINVAL;
    if (B == 0) return 0;
    if (!removed || !acc_counts || !acc_mass) return GI_EINVAL;
    hipLaunchKernelGGL(mask_stats_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, B, removed, grow_state,
                       acc_counts, acc_mass);
    return gi_launch_status();
}
