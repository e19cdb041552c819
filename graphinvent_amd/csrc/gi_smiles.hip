// Molecule strings on the device (gfx950): every one of G generated molecules as a SMILES string — the product of the
// reference's `write_graphs_to_smi` (util.py:520-585: one RWMol, one SanitizeMol and one MolToSmiles per molecule on the
// host).  THE STRING IS A FAITHFUL SPELLING OF THE LABELLED GRAPH in an OpenSMILES subset, NOT RDKit's canonical SMILES:
// no aromaticity perception, no kekulisation, no stereo marks, hydrogen counts from the caller's table or the stored
// segment.  The grammar is written out at gi_mol_smiles in include/graphinvent_amd.h; tests/smiles_model.py is the
// Python specification the bytes are held to.
//
// mol_smiles_kernel  one 256-lane WORKGROUP per molecule:
//   1, 2  gi_read_labelled of gi_molread.h, the front end shared with gi_valence.hip and gi_fingerprint.hip: all waves
//      read the molecule once (fp32 or int8) and check it while they read; in LDS one 128-bit adjacency row per (bond
//      type, node) and the segment entries of every node; n and the bits of GI_MOL_MALFORMED, GI_SMI_SELF_LOOP, _EMPTY;
//   3  one lane per atom: x, the hydrogen count (gi_hydrogen_fill, as gi_mol_valence, or the stored one), GI_SMI_OVER,
//      _AROMATIC and the atom token (at most TOK bytes); the traversal key of an atom = its place in the order by
//      (rank, index); the OR of its rows with the bits moved to key space;
//   4  ONE LANE walks depth-first over the key-space rows, its stack in LDS, the visited set in registers: 2 n + 1 steps
//      at most (every step pushes an atom, pops one, or ends the walk).  It leaves the pre-order, the tree parent, the
//      last child and the end of the subtree of every atom, and the number of components;
//   5  one lane per atom (in pre-order space from here on): the rows once more, moved to pre-order space and split into
//      ring bonds (neither to the parent nor to a child), double and triple bonds; the closing parentheses that follow
//      an atom (LDS integer adds);
//   6  WAVE 0 assigns the ring numbers in pre-order, over the atoms that have a ring bond (a bit mask from 5): lane l
//      owns the numbers l + 1 and l + 65 in registers, a closing finds its number and an opening the smallest free one
//      with two ballots; lane 0 appends the ring tokens of every atom to an LDS text of max_len bytes (counted beyond
//      it, never written beyond it);
//   7  one lane per atom: its byte count, its offset (a sum over the atoms before it), its bytes into the LDS string;
//      the row leaves in 16-byte stores, zero tail included, so nothing has to be cleared before the launch.
// Integer arithmetic only, no global atomics: every output bit is deterministic.  Every loop is bounded by N, Fe, 32
// (the bits of a word) or 2 N + 1; every index is bounded by the dims (i, j < N from an offset < N N Fe; key and
// pre-order indices < n; a ring-text or string offset is compared with max_len before it is used).
// LDS: Fe N 16 B rows + 2 max_len dynamic (<= 16 KB + 16 KB), ~23 KB static: at N = 128, Fe = 4 and the default
// max_len 1552 B that is 34 KB, four workgroups per CU.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned char u8;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int TOK = 12;                                      // '[' 2 letters 'H' 3 digits sign 3 digits ']'
constexpr int NO_STRING = GI_MOL_MALFORMED | GI_SMI_EMPTY | GI_SMI_SELF_LOOP | GI_SMI_AROMATIC | GI_SMI_RING_LIMIT;

struct SmiTables {
    const unsigned short* allowed;                           // [A * C]: bit v = total valence v is allowed
    const i8* order2;                                        // [Fe] twice the bond order
    const i8* h_values;                                      // [H] the stored implicit-H counts (H > 0)
    const i8* charges;                                       // [C] the formal charge of every entry
    const u8* symbols;                                       // [A][2] element symbols, the second byte 0 if there is none
    int A, C, H, stored;
};

struct SmiOut {
    u8* text;
    int* length;
    int* status;
    int* atom_pos;
    int max_len;
};

// v in [0, 999] as decimal digits at p -> the digits written (1 to 3)
__device__ __forceinline__ int put_number(u8* p, int v) {
    int k = 0;
    if (v >= 100) p[k++] = (u8)('0' + v / 100);
    if (v >= 10) p[k++] = (u8)('0' + (v / 10) % 10);
    p[k++] = (u8)('0' + v % 10);
    return k;
}

template <typename T>
__global__ __launch_bounds__(NT) void mol_smiles_kernel(const T* __restrict__ nodes, const T* __restrict__ edges,
                                                        const void* __restrict__ n_nodes, int nn_bytes, int N, int Fn,
                                                        int Fe, SmiTables tb, const int* __restrict__ rank, SmiOut out) {
    extern __shared__ __align__(16) unsigned dyn[];          // adj [Fe][N][4] | the string [max_len] | ring text [max_len]
    __shared__ __align__(16) unsigned krow[MAXN][4];         // key space: bit of every bonded partner
    __shared__ __align__(16) unsigned rrow[MAXN][4], dbl[MAXN][4], tpl[MAXN][4];   // pre-order space: ring / double / triple
    __shared__ GiLabelled st;
    __shared__ u8 tok[MAXN][TOK];
    __shared__ int toklen[MAXN], rk[MAXN], kpos[MAXN], kinv[MAXN];     // by input index; kinv by key
    __shared__ int pre[MAXN], park[MAXN], lastc[MAXN], subk[MAXN], stack[MAXN];   // by key
    __shared__ int ord[MAXN], para[MAXN], closers[MAXN], rstart[MAXN], rlen[MAXN], lens[MAXN];   // by pre-order index
    __shared__ int apos[MAXN];                               // by input index
    __shared__ unsigned ringat[4];                           // the pre-order indices that have a ring bond
    unsigned* adj = dyn;
    u8* str = reinterpret_cast<u8*>(dyn + Fe * N * 4);
    u8* rtx = str + out.max_len;
    const int g = blockIdx.x, tid = threadIdx.x, max_len = out.max_len;
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    for (int i = tid; i < max_len / 16; i += NT) reinterpret_cast<uint4*>(str)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < MAXN) { closers[tid] = 0; apos[tid] = -1; }
    if (tid < 4) ringat[tid] = 0u;

    // ---- 1, 2: read and check; n and the well-formedness bits ---------------------------------------------
    GiLabelledNode me;                                       // me.seen: this lane's node, the OR of its rows
    const int n = gi_read_labelled<false>(nodes + (size_t)g * (N * Fn), edges + (size_t)g * (N * N * Fe), n_nodes,
                                          nn_bytes, g, N, Fn, Fe, tb.A, tb.C, tb.H, tb.order2, tid, adj, st, nullptr, me);
    const bool sound = (st.flags & GI_MOL_MALFORMED) == 0;   // uniform
    const bool mine = sound && tid < n;                      // this lane owns input atom `tid`

    // ---- 3: valence, hydrogens, the atom token; the keys ----------------------------------------------------
    int flags = 0;
    if (mine) {
        const int x = (gi_atom_order2(adj, tb.order2, N, Fe, tid) + 1) >> 1;
        const int a = st.seg_first[0][tid], c = st.seg_first[1][tid];     // a < A, c < C: the row is one-hot
        int h = gi_hydrogen_fill((unsigned)tb.allowed[a * tb.C + c], x);
        if (h < 0) { flags |= GI_SMI_OVER; h = 0; }
        if (tb.stored) h = (int)tb.h_values[st.seg_first[2][tid]];        // < H: the row is one-hot
        if (me.arom) flags |= GI_SMI_AROMATIC;
        const u8 s0 = tb.symbols[2 * a], s1 = tb.symbols[2 * a + 1];
        const int q = (int)tb.charges[c];
        const unsigned org = organic_valences(s0, s1);
        const int implicit = max(gi_hydrogen_fill(org, x), 0);
        u8* p = tok[tid];
        int k = 0;
        if (s0 == 'H' && s1 == 0) h = 0;                     // "[H]" never carries a count
        else if (org && q == 0 && h == implicit) {           // bare
            p[k++] = s0;
            if (s1) p[k++] = s1;
        }
        if (k == 0) {
            p[k++] = '[';
            p[k++] = s0;
            if (s1) p[k++] = s1;
            if (h >= 1) p[k++] = 'H';
            if (h >= 2) k += put_number(p + k, h);           // h <= 127
            if (q) {
                p[k++] = q > 0 ? '+' : '-';
                const int m = q > 0 ? q : -q;                // <= 128
                if (m >= 2) k += put_number(p + k, m);
            }
            p[k++] = ']';
        }
        toklen[tid] = k;
        rk[tid] = rank ? rank[(size_t)g * N + tid] : tid;
    }
    __syncthreads();
    if (mine) {                                              // the key: the place in the order by (rank, index)
        const int r = rk[tid];
        int pos = 0;
        for (int j = 0; j < n; ++j) {
            const int rj = rk[j];
            pos += (rj < r || (rj == r && j < tid)) ? 1 : 0;
        }
        kpos[tid] = pos;                                     // a permutation of [0, n)
        kinv[pos] = tid;
    }
    __syncthreads();
    if (mine) {
        unsigned moved[4] = {0u, 0u, 0u, 0u};
        for (int w = 0; w < 4; ++w) {
            unsigned bits = me.seen[w] & gi_below_word(n, w);
            while (bits) {                                   // at most 32 bits
                const int j = 32 * w + __builtin_ctz(bits);
                bits &= bits - 1;
                const int k = kpos[j];
                for (int u = 0; u < 4; ++u) moved[u] |= (k >> 5) == u ? 1u << (k & 31) : 0u;
            }
        }
        const int k = kpos[tid];
        for (int u = 0; u < 4; ++u) krow[k][u] = moved[u];
    }
    __syncthreads();

    // ---- 4: the walk ---------------------------------------------------------------------------------------
    if (sound && tid == 0) {
        typedef unsigned long long u64;
        const u64 all0 = (u64)gi_below_word(n, 0) | (u64)gi_below_word(n, 1) << 32;
        const u64 all1 = (u64)gi_below_word(n, 2) | (u64)gi_below_word(n, 3) << 32;
        u64 vis0 = 0, vis1 = 0;                              // the visited keys 0 .. 63 and 64 .. 127
        int cnt = 0, comps = 0, sp = 0, p = -1;              // p: the top of the stack (-1: it is empty)
        for (int it = 0; it < 2 * n + 1; ++it) {             // a push, a pop or the end in every step
            u64 c0, c1;
            if (sp == 0) {                                   // a new component starts at the lowest key not yet seen
                c0 = all0 & ~vis0;
                c1 = all1 & ~vis1;
                if ((c0 | c1) == 0) break;
                ++comps;
            } else {
                const uint4 row = *reinterpret_cast<const uint4*>(krow[p]);        // 0 <= p < n
                c0 = ((u64)row.x | (u64)row.y << 32) & all0 & ~vis0;
                c1 = ((u64)row.z | (u64)row.w << 32) & all1 & ~vis1;
                if ((c0 | c1) == 0) {                        // done with p: its subtree ends at the last atom numbered
                    subk[p] = cnt - 1;
                    --sp;
                    p = sp ? stack[sp - 1] : -1;             // 0 < sp <= n
                    continue;
                }
            }
            const int c = c0 ? __builtin_ctzll(c0) : 64 + __builtin_ctzll(c1);      // < n
            if (c0) vis0 |= 1ull << c;
            else vis1 |= 1ull << (c - 64);
            if (p >= 0) lastc[p] = c;
            pre[c] = cnt;                                    // cnt < n: every atom is numbered once
            ord[cnt] = c;
            park[c] = p;
            lastc[c] = -1;
            ++cnt;
            stack[sp++] = c;                                 // sp <= n: every atom is pushed once
            p = c;
        }
        if (comps > 1) atomicOr(&st.flags, GI_SMI_FRAGMENTS);
    }
    if (flags) atomicOr(&st.flags, flags);
    __syncthreads();
    const bool walk = (st.flags & NO_STRING) == 0;           // uniform; the ring limit is not known yet
    const bool atom = walk && tid < n;                       // this lane owns the atom of pre-order index `tid`

    // ---- 5: pre-order space ----------------------------------------------------------------------------------
    int me_in = 0, nonlast = 0;
    if (atom) {
        const int k = ord[tid], pk = park[k];
        me_in = kinv[k];
        para[tid] = pk < 0 ? -1 : pre[pk];
        nonlast = pk >= 0 && lastc[pk] != k;
        if (nonlast) atomicAdd(&closers[subk[k]], 1);        // subk[k] in [tid, n)
    }
    __syncthreads();
    u8 lead = 0;
    if (atom) {
        unsigned ring[4] = {0u, 0u, 0u, 0u}, d2[4] = {0u, 0u, 0u, 0u}, d3[4] = {0u, 0u, 0u, 0u};
        const int pa = para[tid];
        for (int t = 0; t < Fe; ++t) {
            const int o2 = (int)tb.order2[t];
            for (int w = 0; w < 4; ++w) {
                unsigned bits = adj[(t * N + me_in) * 4 + w] & gi_below_word(n, w);
                while (bits) {                               // at most 32 bits
                    const int j = 32 * w + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const int q = pre[kpos[j]];              // j < n
                    const unsigned bit = 1u << (q & 31);
                    const bool tree = q == pa || para[q] == tid || q == tid;
                    for (int u = 0; u < 4; ++u) {
                        const unsigned b = (q >> 5) == u ? bit : 0u;
                        if (!tree) ring[u] |= b;
                        if (o2 == 4) d2[u] |= b;
                        if (o2 == 6) d3[u] |= b;
                    }
                    if (q == pa) lead = o2 == 4 ? '=' : o2 == 6 ? '#' : 0;
                }
            }
        }
        for (int u = 0; u < 4; ++u) { rrow[tid][u] = ring[u]; dbl[tid][u] = d2[u]; tpl[tid][u] = d3[u]; }
        if (ring[0] | ring[1] | ring[2] | ring[3]) atomicOr(&ringat[tid >> 5], 1u << (tid & 31));
        else { rstart[tid] = 0; rlen[tid] = 0; }             // no ring token: stage 6 passes this atom by
    }
    __syncthreads();

    // ---- 6: ring numbers, in pre-order (wave 0) ----------------------------------------------------------------
    if (walk && tid < 64) {
        int own_a = -1, own_b = -1;                          // the ring that holds number tid + 1 / tid + 65
        int roff = 0;
        bool limit = false;
        auto put = [&](u8 b) {
            if (tid == 0 && roff < max_len) rtx[roff] = b;
            ++roff;
        };
        auto put_ring = [&](int num) {                       // 0 <= num <= 99
            if (num >= 10) { put('%'); put((u8)('0' + num / 10)); }
            put((u8)('0' + num % 10));
        };
        for (int wa = 0; wa < 4; ++wa) {                     // the atoms with a ring bond, ascending: bits < n
            unsigned todo = ringat[wa];
            while (todo && !limit) {                         // at most 32 bits
                const int a = 32 * wa + __builtin_ctz(todo);
                todo &= todo - 1;
                const int start = roff;
                const uint4 row4 = *reinterpret_cast<const uint4*>(rrow[a]);
                const unsigned rr[4] = {row4.x, row4.y, row4.z, row4.w};
                for (int w = 0; w < 4; ++w) {                // closings: partners before a
                    unsigned bits = rr[w] & gi_below_word(a, w);
                    while (bits) {
                        const int q = 32 * w + __builtin_ctz(bits);
                        bits &= bits - 1;
                        const int key = q * MAXN + a;
                        const unsigned long long ma = __ballot(own_a == key), mb = __ballot(own_b == key);
                        const int num = ma ? __builtin_ctzll(ma) + 1 : mb ? __builtin_ctzll(mb) + 65 : 0;
                        if (own_a == key) own_a = -1;
                        if (own_b == key) own_b = -1;
                        if (row_bit(dbl[a], q)) put('=');
                        else if (row_bit(tpl[a], q)) put('#');
                        put_ring(num);
                    }
                }
                for (int w = 0; w < 4 && !limit; ++w) {      // openings: partners after a
                    unsigned bits = rr[w] & ~gi_below_word(a + 1, w) & gi_below_word(n, w);
                    while (bits && !limit) {
                        const int q = 32 * w + __builtin_ctz(bits);
                        bits &= bits - 1;
                        const unsigned long long fa = __ballot(own_a < 0), fb = __ballot(tid < 35 && own_b < 0);
                        int num = 0;
                        if (fa) {
                            const int l = __builtin_ctzll(fa);
                            num = l + 1;
                            if (tid == l) own_a = a * MAXN + q;
                        } else if (fb) {
                            const int l = __builtin_ctzll(fb);
                            num = l + 65;
                            if (tid == l) own_b = a * MAXN + q;
                        } else {
                            limit = true;
                        }
                        if (!limit) put_ring(num);
                    }
                }
                if (tid == 0) { rstart[a] = start; rlen[a] = roff - start; }
            }
        }
        if (limit && tid == 0) atomicOr(&st.flags, GI_SMI_RING_LIMIT);
    }
    __syncthreads();
    const bool written = walk && (st.flags & GI_SMI_RING_LIMIT) == 0;    // uniform

    // ---- 7: byte counts, offsets, the string -------------------------------------------------------------------
    const int dot = atom && tid > 0 && para[tid] < 0;
    if (written && tid < n)
        lens[tid] = dot + nonlast + (lead ? 1 : 0) + toklen[me_in] + rlen[tid] + closers[tid];
    __syncthreads();
    int off = 0, total = 0;
    if (written)
        for (int b = 0; b < n; ++b) {                        // <= 128 (8 + 12 + 4 * 127 + 127) bytes: no overflow
            const int l = lens[b];
            off += b < tid ? l : 0;
            total += l;
        }
    const bool fits = written && total <= max_len;           // uniform
    if (fits && tid < n) {                                   // off + lens[tid] <= total <= max_len
        int p = off;
        if (dot) str[p++] = '.';
        if (nonlast) str[p++] = '(';
        if (lead) str[p++] = lead;
        apos[me_in] = p;
        for (int k = 0; k < toklen[me_in]; ++k) str[p++] = tok[me_in][k];
        const int rs = rstart[tid], rl = rlen[tid];          // rs + rl <= the ring text's length <= total <= max_len
        for (int k = 0; k < rl; ++k) str[p++] = rtx[rs + k];
        for (int k = 0; k < closers[tid]; ++k) str[p++] = ')';
    }
    __syncthreads();
    uint4* row = reinterpret_cast<uint4*>(out.text + (size_t)g * max_len);          // 16-byte aligned (checked on the host)
    for (int i = tid; i < max_len / 16; i += NT) row[i] = reinterpret_cast<const uint4*>(str)[i];
    if (tid < N) out.atom_pos[(size_t)g * N + tid] = apos[tid];
    if (tid == 0) {
        out.length[g] = written ? total : 0;
        out.status[g] = st.flags | (written && !fits ? GI_SMI_TRUNCATED : 0);
    }
}

}  // namespace

extern "C" int gi_mol_smiles(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                             const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                             const unsigned short* allowed, const signed char* order2, const signed char* h_values,
                             const signed char* charges, const unsigned char* symbols, int stored_h, const int* rank,
                             int max_len, unsigned char* text, int* length, int* status, int* atom_pos, void* stream) {
    (void)hipGetLastError();
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_types(dtype, n_nodes_bytes)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    if ((stored_h != 0 && stored_h != 1) || (stored_h && n_imp_h == 0)) return GI_EINVAL;
    if (const int rc = gi_smi_check_max_len(max_len)) return rc;
    if (G == 0) return 0;
    if (!nodes || !edges || !allowed || !order2 || (n_imp_h > 0 && !h_values) || !charges || !symbols || !text ||
        !length || !status || !atom_pos || ((uintptr_t)text & 15))
        return GI_EINVAL;
    const SmiTables tb = {allowed, order2, h_values, charges, symbols, n_types, n_charges, n_imp_h, stored_h};
    const SmiOut out = {text, length, status, atom_pos, max_len};
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned) + 2 * (size_t)max_len;                // <= 32 KB
    if (dtype == GI_DTYPE_F32)
        hipLaunchKernelGGL(mol_smiles_kernel<float>, dim3(G), dim3(NT), lds, st, (const float*)nodes,
                           (const float*)edges, n_nodes, n_nodes_bytes, N, Fn, Fe, tb, rank, out);
    else
        hipLaunchKernelGGL(mol_smiles_kernel<i8>, dim3(G), dim3(NT), lds, st, (const i8*)nodes, (const i8*)edges,
                           n_nodes, n_nodes_bytes, N, Fn, Fe, tb, rank, out);
    return gi_launch_status();
}
