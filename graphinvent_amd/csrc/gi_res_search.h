// The matching machinery of gi_resonance.hip as host-device code with no dependency on HIP, so that a plain C++
// compiler can run it on the host against tests/resonance_model.py (tests/test_resonance_cpu.py does):
//   res_search     one breadth-first augmenting-path search with blossom contraction from a free atom: the search of
//                  tests/kekule_read_model.py::match, statement by statement (neighbours in ascending index, the
//                  blossom's atoms queued in ascending index), on a matching that is given.  The matching can be
//                  looked at through a window: two atoms count as free whatever `mate` says, a set of atoms and one
//                  edge are left out of the graph.  Nothing is written but the caller's parent / base / queue bytes;
//   res_match      `match` itself: the greedy pass, then one search per free needing atom (gi_mol_kekulize, one lane);
//   res_doubles / res_singles   the verdicts of gi_mol_resonance for the bonds of one atom: a double bond (a, mate a)
//                  is delocalised iff an augmenting path joins a and mate a once the bond is taken out, a single bond
//                  (u, v) iff one joins mate u and mate v once u and v are taken out; the path and what was taken out
//                  close an alternating cycle, ALL of whose bonds are marked at once.
// A graph: rows [n][4], bit j of row i = candidate bond between i and j (the caller guarantees j < n and no bit i in row
// i).  Bytes: an atom index < n <= 128, or RES_NONE.  An array `x` with stride `st` keeps entry k at x[k * st], so that
// the lanes of a workgroup can interleave their workspaces.  Every loop is bounded by n or by the number of set bits;
// an index read back from the workspace is compared with n before it is used, so no input can make an access leave
// the arrays.
#pragma once

#if defined(__HIPCC__)
#define RES_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RES_HD inline
#endif

constexpr int RES_NONE = 0xff;

RES_HD int res_ctz(unsigned x) { return __builtin_ctz(x); }
RES_HD bool res_bit(const unsigned* m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; }
RES_HD void res_set(unsigned* m, int i) { m[i >> 5] |= 1u << (i & 31); }

// the matching as a search sees it
struct ResView {
    const unsigned char* mate;                               // stride 1
    int f1, f2;                                              // free whatever `mate` says (-1: nobody)
    RES_HD int of(int v) const { return (v == f1 || v == f2) ? RES_NONE : (int)mate[v]; }
};

// -> the free atom reached (parent[] then holds the path back to `root`), or -1.  rm [4]: atoms left out; (ban_a,
// ban_b): an edge left out (-1: none).
RES_HD int res_search(const unsigned* rows, int n, ResView M, const unsigned* rm, int ban_a, int ban_b, int root,
                      unsigned char* parent, unsigned char* base, unsigned char* queue, int st) {
    unsigned used[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < n; ++i) {
        parent[i * st] = (unsigned char)RES_NONE;
        base[i * st] = (unsigned char)i;
    }
    res_set(used, root);
    queue[0] = (unsigned char)root;
    int head = 0, tail = 1;
    while (head < tail) {                                    // tail <= n: an atom is queued once
        const int v = queue[head * st];
        ++head;
        const int mv = M.of(v);
        for (int w = 0; w < 4; ++w) {
            unsigned bits = rows[v * 4 + w] & ~rm[w];
            while (bits) {
                const int to = 32 * w + res_ctz(bits);
                bits &= bits - 1;
                if (to >= n || (v == ban_a && to == ban_b) || (v == ban_b && to == ban_a)) continue;
                if (base[v * st] == base[to * st] || mv == to) continue;
                const int mt = M.of(to);
                if (to == root || (mt < n && parent[mt * st] != RES_NONE)) {
                    // an odd cycle closes: its lowest common base ...
                    unsigned seen[4] = {0u, 0u, 0u, 0u};
                    int a = v, cur = -1;
                    for (int it = 0; it <= n; ++it) {
                        a = base[a * st];
                        res_set(seen, a);
                        const int ma = M.of(a);
                        if (ma >= n) break;
                        a = parent[ma * st];
                        if (a >= n) break;                   // (not reached on a consistent workspace)
                    }
                    int b = to;
                    for (int it = 0; it <= n; ++it) {
                        b = base[b * st];
                        if (res_bit(seen, b)) { cur = b; break; }
                        const int mb = M.of(b);
                        if (mb >= n) break;
                        b = parent[mb * st];
                        if (b >= n) break;
                    }
                    if (cur < 0) return -1;                  // (not reached)
                    // ... the two paths down to it become one blossom
                    unsigned bl[4] = {0u, 0u, 0u, 0u};
                    for (int side = 0; side < 2; ++side) {
                        int x = side ? to : v, child = side ? v : to;
                        for (int it = 0; it < n && base[x * st] != cur; ++it) {
                            const int mx = M.of(x);
                            if (mx >= n) break;              // (not reached)
                            res_set(bl, base[x * st]);
                            res_set(bl, base[mx * st]);
                            parent[x * st] = (unsigned char)child;
                            child = mx;
                            x = parent[mx * st];
                            if (x >= n) return -1;           // (not reached)
                        }
                    }
                    for (int i = 0; i < n; ++i)
                        if (res_bit(bl, base[i * st])) {
                            base[i * st] = (unsigned char)cur;
                            if (!res_bit(used, i)) {
                                res_set(used, i);
                                if (tail < n) queue[tail++ * st] = (unsigned char)i;
                            }
                        }
                } else if (parent[to * st] == RES_NONE) {
                    parent[to * st] = (unsigned char)v;
                    if (mt >= n) return to;
                    res_set(used, mt);
                    if (tail < n) queue[tail++ * st] = (unsigned char)mt;
                }
            }
        }
    }
    return -1;
}

// `match`: a perfect matching of the atoms with a non-empty row -> true, mate [n] (RES_NONE outside), or false.
// counters (or nullptr): greedy pairs, searches, augmentations.
RES_HD bool res_match(const unsigned* rows, int n, unsigned char* mate, unsigned char* parent, unsigned char* base,
                      unsigned char* queue, int* counters) {
    const unsigned none[4] = {0u, 0u, 0u, 0u};
    auto need = [&](int i) { return (rows[i * 4] | rows[i * 4 + 1] | rows[i * 4 + 2] | rows[i * 4 + 3]) != 0u; };
    for (int i = 0; i < n; ++i) mate[i] = (unsigned char)RES_NONE;
    for (int i = 0; i < n; ++i) {                            // the greedy pass
        if (!need(i) || mate[i] != RES_NONE) continue;
        bool done = false;
        for (int w = 0; w < 4 && !done; ++w) {
            unsigned bits = rows[i * 4 + w];
            while (bits && !done) {
                const int j = 32 * w + res_ctz(bits);
                bits &= bits - 1;
                if (j < n && j != i && mate[j] == RES_NONE) {
                    mate[i] = (unsigned char)j;
                    mate[j] = (unsigned char)i;
                    if (counters) ++counters[0];
                    done = true;
                }
            }
        }
    }
    for (int root = 0; root < n; ++root) {
        if (!need(root) || mate[root] != RES_NONE) continue;
        if (counters) ++counters[1];
        const ResView M = {mate, -1, -1};
        int v = res_search(rows, n, M, none, -1, -1, root, parent, base, queue, 1);
        if (v < 0) return false;
        if (counters) ++counters[2];
        for (int it = 0; it < n && v < n; ++it) {            // flip the path
            const int pv = parent[v];
            if (pv >= n) break;                              // (not reached)
            const int nxt = mate[pv];
            mate[v] = (unsigned char)pv;
            mate[pv] = (unsigned char)v;
            v = nxt;
        }
    }
    return true;
}

// One search of gi_mol_resonance and, if it succeeds, the marks of the whole alternating cycle.  `D` has
// mark(a, b) (sets bond a-b both ways) and marked(a, b).
template <class D>
RES_HD bool res_cycle(const unsigned* gp, int n, const unsigned char* mate, int fa, int fb, const unsigned* rm, int ban_a,
                      int ban_b, unsigned char* parent, unsigned char* base, unsigned char* queue, int st, D& d) {
    const ResView M = {mate, fa, fb};
    int v = res_search(gp, n, M, rm, ban_a, ban_b, fa, parent, base, queue, st);
    if (v < 0) return false;
    for (int it = 0; it < n && v < n; ++it) {                // the path: (v, parent v), then parent v's matched bond
        const int pv = parent[v * st];
        if (pv >= n) break;                                  // (not reached)
        d.mark(v, pv);
        const int nxt = M.of(pv);
        if (nxt < n) d.mark(pv, nxt);
        v = nxt;
    }
    return true;
}

// the double bond of atom a (the caller: a in V', a < mate a): -> the number of searches made
template <class D>
RES_HD int res_doubles(const unsigned* gp, int n, const unsigned char* mate, int a, unsigned char* parent,
                       unsigned char* base, unsigned char* queue, int st, D& d) {
    const int b = mate[a];
    if (b >= n || b <= a || d.marked(a, b)) return 0;
    const unsigned none[4] = {0u, 0u, 0u, 0u};
    if (res_cycle(gp, n, mate, a, b, none, a, b, parent, base, queue, st, d)) d.mark(a, b);
    return 1;
}

// the single bonds (u, v), v > u, of atom u in V': only between two atoms whose double bonds are delocalised (all of
// res_doubles has finished), and only those no cycle has marked yet
template <class D>
RES_HD int res_singles(const unsigned* gp, int n, const unsigned char* mate, int u, unsigned char* parent,
                       unsigned char* base, unsigned char* queue, int st, D& d) {
    const int mu = mate[u];
    if (mu >= n || !d.marked(u, mu)) return 0;
    int searches = 0;
    for (int w = 0; w < 4; ++w) {
        unsigned bits = gp[u * 4 + w];
        while (bits) {
            const int v = 32 * w + res_ctz(bits);
            bits &= bits - 1;
            if (v <= u || v >= n || v == mu) continue;
            const int mv = mate[v];
            if (mv >= n || !d.marked(v, mv) || d.marked(u, v)) continue;
            unsigned rm[4] = {0u, 0u, 0u, 0u};
            res_set(rm, u);
            res_set(rm, v);
            ++searches;
            if (res_cycle(gp, n, mate, mu, mv, rm, -1, -1, parent, base, queue, st, d)) {
                d.mark(mu, u);
                d.mark(u, v);
                d.mark(v, mv);
            }
        }
    }
    return searches;
}
