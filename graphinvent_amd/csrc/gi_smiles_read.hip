// SMILES strings into molecules on the device (gfx950): the inverse of gi_smiles.hip on the writer's subset of
// OpenSMILES, what the reference's preprocessing gets from one MolFromSmiles and one graph construction per molecule on
// the host.  NO AROMATIC INPUT AND NO STEREO: a lowercase atom, ':' or (unless they are dropped) '@' '/' '\' give a
// status bit and the all-zero molecule, so that the caller can route the string to RDKit;
// gi_smiles_read_arom with aromatic = 1 (the kernel's AROM instantiation) takes aromatic atoms and ':' instead and
// kekulises them: OUR rule, not RDKit's, tests/kekule_read_model.py is its specification.  Atoms are numbered in string
// order.  The grammar and the status bits are written out at gi_smiles_read in include/graphinvent_amd.h;
// tests/smiles_read_model.py is the Python specification every output byte is held to, stage by stage.
//
// smiles_read_kernel  one 256-lane WORKGROUP per string:
//   0  the string, once, in 16-byte pieces into LDS; without a length it ends at its first zero byte (an LDS min);
//   A  one lane per byte.  A byte is inside a bracket when the last '[' or ']' before it is a '[': two ballots per 64
//      bytes, and per 64-byte word the state it starts in (one lane per word looks back over the words).  Every byte
//      gets its class; a ballot of the atom tokens and a popcount sum per word give each token its index;
//   B  one lane per atom parses its own token and looks its symbol and charge up in the tables;
//   C  ONE LANE walks the bond, branch, ring and dot tokens, 16 classes per LDS read: a branch stack of 128 entries and
//      a ring table of 100 in LDS, the bonds as bits in the 128-bit adjacency rows per bond type (LDS atomics nobody
//      waits for); at most `length` steps, the only serial part;
//   C2 AROM only.  Stage C has put the aromatic-marked bonds (no symbol, or ':', between two aromatic atoms) into one more
//      128-bit row set `arom` instead of `adj`.  One lane per atom: sigma from popcounts, whether the atom needs a double
//      bond, its bit in the need mask (an LDS atomic).  ONE LANE finds a perfect matching of the needing atoms over the
//      candidate rows arom[i] & need: a greedy pass in ascending index, then one breadth-first augmenting-path search with
//      blossom contraction per atom still free (mate / parent / base / queue: byte arrays of 128 in LDS; visited, blossom
//      and ancestor sets: 128-bit masks in LDS; neighbours by ctz over the candidate row).  None: GI_SMR_KEKULE.  All lanes
//      move their arom bits into the double type's row (the mate) and the single type's (the rest).  Bounds: the greedy
//      pass scans at most n rows; at most n / 2 searches, each of which dequeues at most n atoms (an atom is queued once)
//      and contracts at most n blossoms (each takes at least one atom out of the unvisited ones or merges two bases), a
//      contraction costing two ancestor walks and two path markings of at most n steps and one pass over n bases; every
//      byte read from mate / parent / base is masked to 0 .. 127 before it is used as an index;
//   D  one lane per atom: the bond-order sum, the hydrogens (implicit or stated), their entry, the valence;
//   E  all lanes write the node and edge rows from the bit rows (store_bytes of gi_molread.h: 16-byte stores between the
//      ragged ends of the row's address range), zeros included, so nothing has to be cleared before the launch.
// Integer arithmetic only, no global atomics, no scratch: every output bit is deterministic.  Every loop is bounded by
// max_len, N, Fe, the table widths or the 64 bits of a word whatever the bytes hold; every index is bounded before use
// (a byte offset < length <= max_len; an atom index < n <= N; a ring number <= 99; a stack index < 128).
// LDS: Fe N 16 B rows + 2 max_len dynamic (<= 16 KB + 16 KB), ~11 KB static; AROM: 2.7 KB more.
#include "gi_common.h"
#include "gi_molread.h"

namespace {

typedef signed char i8;
typedef unsigned char u8;
typedef unsigned long long u64;

constexpr int NT = GI_MOL_NT;
constexpr int MAXN = GI_MAX_NODES;
constexpr int MAXW = GI_SMI_MAX_LEN / 64;                    // 64-byte words of the longest string
constexpr int DEPTH = 128, RINGS = 100, SATURATE = 1000;
constexpr int ERR = GI_SMR_ERROR;
enum : u8 { T_SKIP, T_ATOM, T_BOND1, T_BOND2, T_BOND3, T_PERCENT, T_OPEN, T_CLOSE, T_DOT, T_BONDA, T_DIGIT = 16 };   // a digit d: T_DIGIT + d
constexpr u8 NONE = 0xff;                                    // mate / parent: nobody

struct ReadTables {
    const unsigned short* allowed;                           // [A * C]: bit v = total valence v is allowed
    const i8* order2;                                        // [Fe] twice the bond order
    const i8* h_values;                                      // [H] the implicit-H counts (H > 0)
    const i8* charges;                                       // [C] the formal charge of every entry
    const u8* symbols;                                       // [A][2] element symbols, the second byte 0 if there is none
    int A, C, H;
};

struct ReadOut {
    i8* nodes;
    i8* edges;
    int* n_nodes;
    int* status;
    int* atom_pos;
};

__device__ __forceinline__ bool is_digit(u8 b) { return b >= '0' && b <= '9'; }
__device__ __forceinline__ bool is_upper(u8 b) { return b >= 'A' && b <= 'Z'; }
__device__ __forceinline__ bool is_lower(u8 b) { return b >= 'a' && b <= 'z'; }

template <bool AROM>
__global__ __launch_bounds__(NT) void smiles_read_kernel(const u8* __restrict__ text, const int* __restrict__ length,
                                                         int max_len, int N, int Fn, int Fe, ReadTables tb,
                                                         int none_chirality, int drop_stereo, ReadOut out) {
    extern __shared__ __align__(16) unsigned dyn[];          // adj [Fe][N][4] | the string [max_len] | classes [max_len]
    __shared__ u64 openw[MAXW], closew[MAXW], atomw[MAXW];   // per 64-byte word: the '[' bytes, the ']' bytes, the atom tokens
    __shared__ int carry[MAXW], prefix[MAXW];                // the bracket state a word starts in; the atoms before it
    __shared__ __align__(16) unsigned anyrow[MAXN][4];       // bit of every bonded partner
    __shared__ int start[MAXN], a_idx[MAXN], c_idx[MAXN], h_idx[MAXN], h_stated[MAXN];   // h_stated -1: a bare atom
    __shared__ int stack[DEPTH], ring_open[RINGS], root[MAXN];       // root: the union-find over segments
    __shared__ int flags_sh, len_sh, atoms_sh;
    __shared__ __align__(16) unsigned arom[AROM ? MAXN : 1][4];      // AROM: bit of every aromatic-marked partner
    __shared__ u8 is_arom[AROM ? MAXN : 1], mate[AROM ? MAXN : 1], par[AROM ? MAXN : 1], bas[AROM ? MAXN : 1], que[AROM ? MAXN : 1];
    __shared__ unsigned needm[AROM ? 4 : 1], usedm[AROM ? 4 : 1], blosm[AROM ? 4 : 1], seenm[AROM ? 4 : 1];      // the needing atoms; the sets of one search
    unsigned* adj = dyn;
    u8* str = reinterpret_cast<u8*>(dyn + Fe * N * 4);
    u8* cls = str + max_len;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int A = tb.A, C = tb.C, H = tb.H;

    // ---- 0: the string ---------------------------------------------------------------------------------------
    for (int i = tid; i < Fe * N * 4; i += NT) adj[i] = 0u;
    for (int i = tid; i < MAXN * 4; i += NT) (&anyrow[0][0])[i] = 0u;
    if (tid < RINGS) ring_open[tid] = -1;
    if (tid < MAXN) root[tid] = tid;
    if constexpr (AROM) {
        for (int i = tid; i < MAXN * 4; i += NT) (&arom[0][0])[i] = 0u;
        if (tid < MAXN) { mate[tid] = NONE; is_arom[tid] = 0; }
        if (tid < 4) needm[tid] = 0u;
    }
    if (tid == 0) { flags_sh = 0; len_sh = max_len; atoms_sh = 0; }
    __syncthreads();
    const int given = length ? length[g] : 0;
    const bool bad_length = length && (given < 0 || given > max_len);
    const int load = length ? (bad_length ? 0 : given) : max_len;
    const uint4* row4 = reinterpret_cast<const uint4*>(text + (size_t)g * max_len);   // 16-byte aligned (checked on the host)
    for (int i = tid; i < (load + 15) / 16; i += NT) {       // (load + 15) / 16 <= max_len / 16
        const uint4 w = row4[i];
        reinterpret_cast<uint4*>(str)[i] = w;
        if (!length) {
            const unsigned v[4] = {w.x, w.y, w.z, w.w};
            int first = 16;
            for (int k = 15; k >= 0; --k)
                if (((v[k >> 2] >> ((k & 3) * 8)) & 0xffu) == 0u) first = k;
            if (first < 16) atomicMin(&len_sh, 16 * i + first);
        }
    }
    __syncthreads();
    const int len = length ? load : len_sh;                  // uniform, 0 <= len <= max_len
    const int words = (len + 63) / 64;                       // <= MAXW
    int flags = 0;
    if (tid == 0) flags = bad_length ? GI_SMR_SYNTAX : len == 0 ? GI_SMR_EMPTY : 0;

    // ---- A: one lane per byte ------------------------------------------------------------------------------------
    for (int base = 0; base < words * 64; base += NT) {      // uniform trip count: every lane of a wave meets the ballots
        const int pos = base + tid, w = pos >> 6;
        const u8 ch = pos < len ? str[pos] : 0;
        const u64 mo = __ballot(ch == '['), mc = __ballot(ch == ']');
        if (lane == 0 && w < words) { openw[w] = mo; closew[w] = mc; }
    }
    __syncthreads();
    if (tid < words) {                                       // the last bracket byte before this word: at most MAXW steps
        int st = 0;
        for (int w = tid - 1; w >= 0; --w) {
            const u64 o = openw[w], m = o | closew[w];
            if (m) { st = (int)((o >> (63 - __builtin_clzll(m))) & 1ull); break; }
        }
        carry[tid] = st;
    }
    __syncthreads();
    for (int base = 0; base < words * 64; base += NT) {
        const int pos = base + tid, w = pos >> 6;
        bool is_atom = false;
        if (pos < len) {
            const u8 ch = str[pos], before = pos > 0 ? str[pos - 1] : 0;
            const u64 o = openw[w], below = (o | closew[w]) & ((1ull << lane) - 1ull);
            const bool inside = below ? (o >> (63 - __builtin_clzll(below))) & 1ull : carry[w] != 0;
            u8 c = T_SKIP;
            if (ch == '[') {
                if (inside) flags |= GI_SMR_SYNTAX;
                else c = T_ATOM;
            } else if (ch == ']') {
                if (!inside) flags |= GI_SMR_SYNTAX;
            } else if (inside) {
            } else if (ch == 'B' || ch == 'C' || ch == 'N' || ch == 'O' || ch == 'P' || ch == 'S' || ch == 'F' || ch == 'I') {
                c = T_ATOM;
            } else if ((ch == 'l' && before == 'C') || (ch == 'r' && before == 'B')) {
            } else if (is_upper(ch)) {
                flags |= GI_SMR_SYNTAX;
            } else if (ch == 'b' || ch == 'c' || ch == 'n' || ch == 'o' || ch == 'p' || ch == 's' || ch == ':') {
                if constexpr (AROM) c = ch == ':' ? T_BONDA : T_ATOM;
                else flags |= GI_SMR_AROMATIC;
            } else if (ch == '/' || ch == '\\') {
                flags |= drop_stereo ? GI_SMR_STEREO_DROPPED : GI_SMR_STEREO;
                c = T_BOND1;
            } else if (ch == '$' || ch == '*') {
                flags |= GI_SMR_UNSUPPORTED;
            } else if (ch == '-') c = T_BOND1;
            else if (ch == '=') c = T_BOND2;
            else if (ch == '#') c = T_BOND3;
            else if (is_digit(ch)) c = (u8)(T_DIGIT + (ch - '0'));
            else if (ch == '%') c = T_PERCENT;
            else if (ch == '(') c = T_OPEN;
            else if (ch == ')') c = T_CLOSE;
            else if (ch == '.') c = T_DOT;
            else flags |= GI_SMR_SYNTAX;
            cls[pos] = c;
            is_atom = c == T_ATOM;
        }
        const u64 ma = __ballot(is_atom);
        if (lane == 0 && w < words) atomw[w] = ma;
    }
    __syncthreads();
    if (tid < words) {                                       // the atoms before this word: at most MAXW steps
        int sum = 0;
        for (int w = 0; w < tid; ++w) sum += __popcll(atomw[w]);
        prefix[tid] = sum;
        if (tid == words - 1) atoms_sh = sum + __popcll(atomw[tid]);
    }
    __syncthreads();
    const int n = atoms_sh;                                  // uniform
    const bool fits = n <= N;
    if (!fits && tid == 0) flags |= GI_SMR_TOO_MANY;
    if (fits && tid < words) {
        int idx = prefix[tid];
        u64 m = atomw[tid];
        while (m) {                                          // at most 64 bits; idx < n <= N
            start[idx++] = 64 * tid + __builtin_ctzll(m);
            m &= m - 1;
        }
    }
    __syncthreads();

    // ---- B: one lane per atom parses its token ---------------------------------------------------------------
    if (fits && tid < n) {
        const int k = start[tid];                            // < len
        auto at = [&](int j) -> u8 { return j < len ? str[j] : (u8)0; };
        int f = 0, h = -1, q = 0;
        u8 s0 = 0, s1 = 0;
        bool small = false;                                  // AROM: the symbol starts with a small letter
        if (str[k] != '[') {
            s0 = str[k];
            small = AROM && is_lower(s0);                    // one of b c n o p s: stage A made it a token
            if (small) s0 = (u8)(s0 - 32);
            else s1 = (s0 == 'C' && at(k + 1) == 'l') ? 'l' : (s0 == 'B' && at(k + 1) == 'r') ? 'r' : 0;
        } else {
            int j = k + 1;
            h = 0;
            const u8 l0 = at(j), l1 = is_lower(at(j + 1)) ? at(j + 1) : (u8)0;  // AROM: b c n o p s se as, looked up capitalised
            small = AROM && is_lower(l0);
            const bool known = small && (l1 ? (l0 == 's' && l1 == 'e') || (l0 == 'a' && l1 == 's')
                                            : l0 == 'b' || l0 == 'c' || l0 == 'n' || l0 == 'o' || l0 == 'p' || l0 == 's');
            if (is_digit(at(j)) || at(j) == '*') f = GI_SMR_UNSUPPORTED;        // an isotope, the wildcard
            else if (is_lower(at(j)) && !known) f = AROM ? GI_SMR_SYNTAX : GI_SMR_AROMATIC;
            else if (!is_upper(at(j)) && !known) f = GI_SMR_SYNTAX;
            else {
                s0 = known ? (u8)(at(j++) - 32) : at(j++);
                if (is_lower(at(j))) s1 = at(j++);
                if (at(j) == '@') {
                    while (at(j) == '@') ++j;                // ends at the end of the string at the latest
                    f |= drop_stereo ? GI_SMR_STEREO_DROPPED : GI_SMR_STEREO;
                }
                if (at(j) == 'H') {
                    ++j;
                    h = 1;
                    if (is_digit(at(j))) {
                        h = 0;
                        while (is_digit(at(j))) h = min(h * 10 + (at(j++) - '0'), SATURATE);
                    }
                }
                bool done = false;
                if (at(j) == '+' || at(j) == '-') {
                    const u8 sign = at(j++);
                    if (at(j) == sign) { f |= GI_SMR_UNSUPPORTED; done = true; }   // "++" / "--"
                    else {
                        int m = 1;
                        if (is_digit(at(j))) {
                            m = 0;
                            while (is_digit(at(j))) m = min(m * 10 + (at(j++) - '0'), SATURATE);
                        }
                        q = sign == '+' ? m : -m;
                    }
                }
                if (!done) {
                    if (at(j) == ':') f |= GI_SMR_UNSUPPORTED;                  // an atom class
                    else if (at(j) != ']') f |= GI_SMR_SYNTAX;
                }
            }
        }
        if (!(f & ERR)) {
            int a = -1, c = -1;
            for (int e = A - 1; e >= 0; --e)
                if (tb.symbols[2 * e] == s0 && tb.symbols[2 * e + 1] == s1) a = e;
            for (int e = C - 1; e >= 0; --e)
                if ((int)tb.charges[e] == q) c = e;
            if (a < 0) f |= GI_SMR_ELEMENT;
            if (c < 0) f |= GI_SMR_CHARGE;
            a_idx[tid] = max(a, 0);
            c_idx[tid] = max(c, 0);
        }
        h_stated[tid] = h;
        if constexpr (AROM) {
            is_arom[tid] = small;
            if (small) f |= GI_SMR_KEKULIZED;                // informational; taken back at the end under an error bit
        }
        flags |= f;
    }
    if (flags) atomicOr(&flags_sh, flags);
    __syncthreads();
    const bool parsed = fits && len > 0 && !bad_length && (flags_sh & ERR) == 0;          // uniform
    __syncthreads();                                         // flags_sh is read by all before the walk changes it

    // ---- C: the walk -------------------------------------------------------------------------------------------
    // The classes come 16 at a time (one LDS read per piece is the loop's only carried latency); the bond bits leave as
    // LDS atomics whose result nobody waits for.  A bond along the chain joins a new atom to its own segment (the atoms
    // between two dots), so only a ring bond between two segments can merge components: a union-find over segments.
    if (parsed && tid == 0) {
        int t1 = -1, t2 = -1, t3 = -1;
        for (int t = Fe - 1; t >= 0; --t) {
            const int o2 = (int)tb.order2[t];
            t1 = o2 == 2 ? t : t1;
            t2 = o2 == 4 ? t : t2;
            t3 = o2 == 6 ? t : t3;
        }
        auto find = [&](int x) {
            for (int it = 0; it < N && root[x] != x; ++it) x = root[x];          // root[x] <= x: it ends within n steps
            return x;
        };
        auto set_bond = [&](int o, int a, int b) -> int {    // a != b < n, not bonded yet; o in 1 .. 3 (AROM: 0 none, 4 ':')
            if constexpr (AROM) {
                const bool both = is_arom[a] && is_arom[b];
                if (o == 4 && !both) return GI_SMR_UNSUPPORTED;
                if ((o == 0 || o == 4) && both) {            // aromatic-marked: stage C2 gives it its type
                    atomicOr(&arom[a][b >> 5], 1u << (b & 31));
                    atomicOr(&arom[b][a >> 5], 1u << (a & 31));
                    atomicOr(&anyrow[a][b >> 5], 1u << (b & 31));
                    atomicOr(&anyrow[b][a >> 5], 1u << (a & 31));
                    return 0;
                }
                o = o ? o : 1;
            }
            const int t = o == 1 ? t1 : o == 2 ? t2 : t3;
            if (t < 0) return GI_SMR_BOND_ORDER;
            atomicOr(&adj[(t * N + a) * 4 + (b >> 5)], 1u << (b & 31));
            atomicOr(&adj[(t * N + b) * 4 + (a >> 5)], 1u << (a & 31));
            atomicOr(&anyrow[a][b >> 5], 1u << (b & 31));
            atomicOr(&anyrow[b][a >> 5], 1u << (a & 31));
            return 0;
        };
        int sp = 0, prev = -1, cur = 0, segments = 0, joins = 0, pending = 0, atoms = 0, err = 0;
        int percent = 0, tens = 0, open_rings = 0;          // cur: the segment of prev; percent: the digits of "%nn" seen
        bool after_open = false;
        const uint4* cls4 = reinterpret_cast<const uint4*>(cls);                  // 16-byte aligned: max_len % 16 == 0
        for (int piece = 0; piece < (len + 15) / 16 && !err; ++piece) {
            const uint4 q = cls4[piece];
            u64 lo = (u64)q.x | (u64)q.y << 32, hi = (u64)q.z | (u64)q.w << 32;
            const int left = min(16, len - 16 * piece);      // the classes behind the string were never written
            for (int b = 0; b < left && !err; ++b) {
                const int t = (int)(lo & 0xffull);
                lo = lo >> 8 | hi << 56;
                hi >>= 8;
                if (t == T_SKIP) continue;                   // never between '%' and its digits: stage A would have objected
                int ring = -1;
                if (percent) {
                    if (t < T_DIGIT) err = GI_SMR_SYNTAX;
                    else if (percent == 1) { tens = 10 * (t - T_DIGIT); percent = 2; }
                    else { ring = tens + (t - T_DIGIT); percent = 0; }
                } else if (t == T_ATOM) {                    // atoms < n: the tokens were counted from the same classes
                    const int me = atoms++;
                    if (prev >= 0) err = set_bond(AROM || pending ? pending : 1, prev, me);   // a new atom has no bond yet
                    else {
                        if (pending) err = GI_SMR_SYNTAX;
                        cur = segments++;                    // < n
                    }
                    prev = me;
                    pending = 0;
                } else if (t == T_BOND1 || t == T_BOND2 || t == T_BOND3 || (AROM && t == T_BONDA)) {
                    if (pending || prev < 0) err = GI_SMR_SYNTAX;
                    pending = t == T_BOND1 ? 1 : t == T_BOND2 ? 2 : t == T_BOND3 ? 3 : 4;
                } else if (t >= T_DIGIT) {
                    ring = t - T_DIGIT;
                } else if (t == T_PERCENT) {
                    percent = 1;
                } else if (t == T_OPEN) {
                    if (prev < 0 || pending || after_open || sp == DEPTH) err = GI_SMR_SYNTAX;
                    else stack[sp++] = prev | cur << 8;
                } else if (t == T_CLOSE) {
                    if (sp == 0 || pending || after_open) err = GI_SMR_SYNTAX;
                    else {
                        const int e = stack[--sp];
                        prev = e & 0xff;
                        cur = e >> 8;
                    }
                } else {                                     // T_DOT
                    if (prev < 0 || pending) err = GI_SMR_SYNTAX;
                    prev = -1;
                }
                if (ring >= 0) {                             // 0 <= ring <= 99
                    if (prev < 0) err = GI_SMR_SYNTAX;
                    else {
                        const int e = ring_open[ring];       // atom | segment << 8 | bond order << 16, -1: closed
                        if (e >= 0) {
                            const int other = e & 0xff, seg = (e >> 8) & 0xff, o = e >> 16;
                            ring_open[ring] = -1;
                            --open_rings;
                            if (o && pending && o != pending) err = GI_SMR_RING_ORDER;
                            else if (other == prev) err = GI_SMR_SELF_LOOP;
                            else if (row_bit(anyrow[other], prev)) err = GI_SMR_MULTI_BOND;
                            else err = set_bond(pending ? pending : o ? o : AROM ? 0 : 1, other, prev);
                            if (!err && seg != cur) {
                                const int ra = find(seg), rb = find(cur);
                                if (ra != rb) {
                                    root[max(ra, rb)] = min(ra, rb);
                                    ++joins;
                                }
                            }
                        } else {
                            ring_open[ring] = prev | cur << 8 | pending << 16;
                            ++open_rings;
                        }
                        pending = 0;
                    }
                }
                after_open = t == T_OPEN;
            }
        }
        if (!err) {
            if (percent || sp || pending) err = GI_SMR_SYNTAX;
            else if (open_rings) err = GI_SMR_RING_OPEN;
            else if (segments - joins > 1) err = GI_SMR_FRAGMENTS;               // informational
        }
        if (err) atomicOr(&flags_sh, err);
    }
    __syncthreads();
    bool walked = parsed && (flags_sh & ERR) == 0;           // uniform
    __syncthreads();

    // ---- C2: the Kekule structure of the aromatic-marked bonds (AROM) ------------------------------------------------
    if constexpr (AROM) {
        int t1 = -1, t2 = -1;
        for (int t = Fe - 1; t >= 0; --t) {
            const int o2 = (int)tb.order2[t];
            t1 = o2 == 2 ? t : t1;
            t2 = o2 == 4 ? t : t2;
        }
        if (walked && tid < n && is_arom[tid]) {             // who needs a double bond
            int o2 = gi_atom_order2(adj, tb.order2, N, Fe, tid);
            for (int w = 0; w < 4; ++w) o2 += 2 * __popc(arom[tid][w]);
            const int h = h_stated[tid];
            const int x = ((o2 + 1) >> 1) + (h < 0 ? 0 : h);             // sigma, with the stated hydrogens of a bracket atom
            const unsigned ok = h < 0 ? organic_valences((u8)(str[start[tid]] - 32), 0)
                                      : (unsigned)tb.allowed[a_idx[tid] * C + c_idx[tid]];
            if (x <= 15 && !((ok >> x) & 1u) && (ok >> x) != 0u) atomicOr(&needm[tid >> 5], 1u << (tid & 31));
        }
        __syncthreads();
        if (walked && tid == 0) {                            // the matching
            const unsigned nd0 = needm[0], nd1 = needm[1], nd2 = needm[2], nd3 = needm[3];
            auto need_word = [&](int w) { return w == 0 ? nd0 : w == 1 ? nd1 : w == 2 ? nd2 : nd3; };   // no array: no scratch
            auto bit = [](const unsigned* m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; };
            auto put = [](unsigned* m, int i) { m[i >> 5] |= 1u << (i & 31); };
#pragma unroll
            for (int w0 = 0; w0 < 4; ++w0) {                 // greedy: the lowest free candidate of every needing atom
                unsigned m = need_word(w0);
                while (m) {
                    const int i = 32 * w0 + __builtin_ctz(m);
                    m &= m - 1;
                    if (mate[i] != NONE) continue;
                    bool done = false;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        unsigned c = done ? 0u : arom[i][w] & need_word(w);
                        while (c) {
                            const int j = 32 * w + __builtin_ctz(c);
                            c &= c - 1;
                            if (mate[j] == NONE) {
                                mate[i] = (u8)j;
                                mate[j] = (u8)i;
                                done = true;
                                break;
                            }
                        }
                    }
                }
            }
            bool perfect = true;
#pragma unroll
            for (int w0 = 0; w0 < 4; ++w0) {                 // one search per atom still free
                unsigned roots = need_word(w0);
                while (roots && perfect) {
                    const int rt = 32 * w0 + __builtin_ctz(roots);
                    roots &= roots - 1;
                    if (mate[rt] != NONE) continue;
                    for (int i = 0; i < n; ++i) { par[i] = NONE; bas[i] = (u8)i; }
                    for (int w = 0; w < 4; ++w) usedm[w] = 0u;
                    put(usedm, rt);
                    que[0] = (u8)rt;
                    int head = 0, tail = 1, found = -1;
                    while (head < tail && found < 0) {       // tail <= n: an atom is queued once
                        const int v = que[head++] & 127;
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            unsigned c = found < 0 ? arom[v][w] & need_word(w) : 0u;
                            while (c && found < 0) {
                                const int to = 32 * w + __builtin_ctz(c);
                                c &= c - 1;
                                if (bas[v] == bas[to] || mate[v] == to) continue;
                                const int mt = mate[to];
                                if (to == rt || (mt != NONE && par[mt & 127] != NONE)) {     // an odd cycle: contract it
                                    for (int k = 0; k < 4; ++k) seenm[k] = blosm[k] = 0u;
                                    int a = v, cur = -1;
                                    for (int it = 0; it <= n; ++it) {                        // the ancestors of v's base
                                        a = bas[a] & 127;
                                        put(seenm, a);
                                        if (mate[a] == NONE) break;
                                        a = par[mate[a] & 127] & 127;
                                    }
                                    a = to;
                                    for (int it = 0; it <= n; ++it) {                        // the first of them above to
                                        a = bas[a] & 127;
                                        if (bit(seenm, a)) { cur = a; break; }
                                        a = par[mate[a] & 127] & 127;
                                    }
                                    if (cur < 0) continue;                                   // (never: both lie in one tree)
                                    for (int side = 0; side < 2; ++side) {
                                        int x = side ? to : v, child = side ? v : to;
                                        for (int it = 0; it < n && bas[x] != cur; ++it) {
                                            const int mx = mate[x] & 127;
                                            put(blosm, bas[x] & 127);
                                            put(blosm, bas[mx] & 127);
                                            par[x] = (u8)child;
                                            child = mx;
                                            x = par[mx] & 127;
                                        }
                                    }
                                    for (int i = 0; i < n; ++i)
                                        if (bit(blosm, bas[i] & 127)) {
                                            bas[i] = (u8)cur;
                                            if (!bit(usedm, i) && tail < MAXN) {
                                                put(usedm, i);
                                                que[tail++] = (u8)i;
                                            }
                                        }
                                } else if (par[to] == NONE) {
                                    par[to] = (u8)v;
                                    if (mt == NONE) found = to;
                                    else if (tail < MAXN) {
                                        put(usedm, mt);
                                        que[tail++] = (u8)mt;
                                    }
                                }
                            }
                        }
                    }
                    if (found < 0) perfect = false;
                    int v = found;
                    for (int it = 0; it < n && v >= 0 && v != NONE; ++it) {      // flip the path found -> rt
                        const int pv = par[v] & 127, next = mate[pv];
                        mate[v] = (u8)pv;
                        mate[pv] = (u8)v;
                        v = next;
                    }
                }
            }
            if (!perfect) atomicOr(&flags_sh, GI_SMR_KEKULE);
        }
        __syncthreads();
        walked = walked && (flags_sh & ERR) == 0;            // uniform
        __syncthreads();                                     // flags_sh is read by all before a missing type changes it
        if (walked && tid < n) {                             // the aromatic-marked bonds get their types: row tid is this lane's
            const int m = mate[tid];
            int f = 0;
            for (int w = 0; w < 4; ++w) {
                const unsigned bits = arom[tid][w];
                const unsigned dbl = (m != NONE && (m >> 5) == w) ? bits & (1u << (m & 31)) : 0u, sgl = bits & ~dbl;
                if (dbl) {
                    if (t2 < 0) f = GI_SMR_BOND_ORDER;
                    else adj[(t2 * N + tid) * 4 + w] |= dbl;
                }
                if (sgl) {
                    if (t1 < 0) f = GI_SMR_BOND_ORDER;
                    else adj[(t1 * N + tid) * 4 + w] |= sgl;
                }
            }
            if (f) atomicOr(&flags_sh, f);
        }
        __syncthreads();
        walked = walked && (flags_sh & ERR) == 0;            // uniform
        __syncthreads();
    }

    // ---- D: one lane per atom: hydrogens, their entry, the valence -----------------------------------------------
    if (walked && tid < n) {
        const int x = (gi_atom_order2(adj, tb.order2, N, Fe, tid) + 1) >> 1;
        int h = h_stated[tid], f = 0;
        if (h < 0) {                                         // bare: the OpenSMILES implicit count
            const int k = start[tid];
            const u8 s0 = AROM && is_lower(str[k]) ? (u8)(str[k] - 32) : str[k];           // a bare aromatic symbol, capitalised
            const u8 s1 = (k + 1 < len && ((s0 == 'C' && str[k + 1] == 'l') || (s0 == 'B' && str[k + 1] == 'r'))) ? str[k + 1] : 0;
            h = max(gi_hydrogen_fill(organic_valences(s0, s1), x), 0);    // the writer's `implicit`
        }
        if (H > 0) {
            int e = -1;
            for (int k = H - 1; k >= 0; --k)
                if ((int)tb.h_values[k] == h) e = k;
            if (e < 0) f |= GI_SMR_HCOUNT;
            h_idx[tid] = max(e, 0);
        }
        if (gi_hydrogen_fill((unsigned)tb.allowed[a_idx[tid] * C + c_idx[tid]], x) < 0) f |= GI_SMR_OVER;
        if (f) atomicOr(&flags_sh, f);
    }
    __syncthreads();
    int status = flags_sh;
    if (AROM && (status & ERR)) status &= ~GI_SMR_KEKULIZED; // set when the string had an aromatic atom AND was read
    const bool good = walked && (status & ERR) == 0;         // uniform

    // ---- E: the rows ---------------------------------------------------------------------------------------------
    const int o_c = A, o_h = A + C, o_x = A + C + H;          // o_x <= Fn, none_chirality < Fn - o_x (checked on the host)
    store_bytes(out.nodes + (size_t)g * N * Fn, N * Fn, tid, N, 1, Fn,
                [&](int i, int) { return good && i < n ? i : -1; },
                [&](int i, int f) {
                    return (f == a_idx[i] || f == o_c + c_idx[i] || (H > 0 && f == o_h + h_idx[i]) ||
                            (o_x < Fn && f == o_x + none_chirality)) ? 1 : 0;
                });
    store_bytes(out.edges + (size_t)g * N * N * Fe, N * N * Fe, tid, N, N, Fe,
                [&](int i, int j) {
                    if (!good || !row_bit(anyrow[i], j)) return -1;
                    int type = -1;
                    for (int t = Fe - 1; t >= 0; --t)
                        if (row_bit(adj + (t * N + i) * 4, j)) type = t;
                    return type;
                },
                [&](int s, int t) { return s == t ? 1 : 0; });
    if (tid < N) out.atom_pos[(size_t)g * N + tid] = good && tid < n ? start[tid] : -1;
    if (tid == 0) {
        out.n_nodes[g] = good || (status & GI_SMR_TOO_MANY) ? n : 0;
        out.status[g] = status;
    }
}

}  // namespace

static int smiles_read_launch(int G, int N, int Fn, int Fe, const unsigned char* text, const int* length, int max_len,
                              int n_types, int n_charges, int n_imp_h, const unsigned short* allowed,
                              const signed char* order2, const signed char* h_values, const signed char* charges,
                              const unsigned char* symbols, int none_chirality, int drop_stereo, int aromatic,
                              signed char* nodes, signed char* edges, int* n_nodes, int* status, int* atom_pos,
                              void* stream) {
    (void)hipGetLastError();
    if (aromatic != 0 && aromatic != 1) return GI_EINVAL;
    if (const int rc = gi_mol_check_dims(G, N, Fn, Fe)) return rc;
    if (const int rc = gi_mol_check_segments(n_types, n_charges, n_imp_h, Fn)) return rc;
    const int rest = Fn - (n_types + n_charges + n_imp_h);
    if (none_chirality < 0 || (rest > 0 && none_chirality >= rest)) return GI_EINVAL;
    if (drop_stereo != 0 && drop_stereo != 1) return GI_EINVAL;
    if (const int rc = gi_smi_check_max_len(max_len)) return rc;
    if (G == 0) return 0;
    if (!text || !allowed || !order2 || (n_imp_h > 0 && !h_values) || !charges || !symbols || !nodes || !edges ||
        !n_nodes || !status || !atom_pos || ((uintptr_t)text & 15))
        return GI_EINVAL;
    const ReadTables tb = {allowed, order2, h_values, charges, symbols, n_types, n_charges, n_imp_h};
    const ReadOut out = {nodes, edges, n_nodes, status, atom_pos};
    const size_t lds = (size_t)Fe * N * 4 * sizeof(unsigned) + 2 * (size_t)max_len;                // <= 32 KB
    if (aromatic)
        hipLaunchKernelGGL(smiles_read_kernel<true>, dim3(G), dim3(NT), lds, (hipStream_t)stream, text, length, max_len,
                           N, Fn, Fe, tb, none_chirality, drop_stereo, out);
    else
        hipLaunchKernelGGL(smiles_read_kernel<false>, dim3(G), dim3(NT), lds, (hipStream_t)stream, text, length, max_len,
                           N, Fn, Fe, tb, none_chirality, drop_stereo, out);
    return gi_launch_status();
}

extern "C" int gi_smiles_read(int G, int N, int Fn, int Fe, const unsigned char* text, const int* length, int max_len,
                              int n_types, int n_charges, int n_imp_h, const unsigned short* allowed,
                              const signed char* order2, const signed char* h_values, const signed char* charges,
                              const unsigned char* symbols, int none_chirality, int drop_stereo, signed char* nodes,
                              signed char* edges, int* n_nodes, int* status, int* atom_pos, void* stream) {
    return smiles_read_launch(G, N, Fn, Fe, text, length, max_len, n_types, n_charges, n_imp_h, allowed, order2, h_values,
                              charges, symbols, none_chirality, drop_stereo, 0, nodes, edges, n_nodes, status, atom_pos,
                              stream);
}

extern "C" int gi_smiles_read_arom(int G, int N, int Fn, int Fe, const unsigned char* text, const int* length,
                                   int max_len, int n_types, int n_charges, int n_imp_h, const unsigned short* allowed,
                                   const signed char* order2, const signed char* h_values, const signed char* charges,
                                   const unsigned char* symbols, int none_chirality, int drop_stereo, int aromatic,
                                   signed char* nodes, signed char* edges, int* n_nodes, int* status, int* atom_pos,
                                   void* stream) {
    return smiles_read_launch(G, N, Fn, Fe, text, length, max_len, n_types, n_charges, n_imp_h, allowed, order2, h_values,
                              charges, symbols, none_chirality, drop_stereo, aromatic, nodes, edges, n_nodes, status,
                              atom_pos, stream);
}
