// The host side of gi_mol_resonance and gi_mol_kekulize (the argument checks) and the host-device matching code of
// csrc/gi_res_search.h under a host sanitizer, without a device: every call of an entry point below returns before
// anything is launched, and the searches run on the host.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igraphinvent_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         graphinvent_amd/csrc/gi_resonance.hip tools/resonance_args.cpp -o /tmp/resonance_args && /tmp/resonance_args
#include <cstdio>
#include <vector>

#include "gi_res_search.h"
#include "graphinvent_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

struct Args {
    int G = 0, N = 13, Fn = 8, Fe = 3, dtype = GI_DTYPE_I8, nn_bytes = 1, A = 5, C = 3, H = 0;
    const void* buf = nullptr;
    int* out = nullptr;
    signed char* edges_out = nullptr;
};

static int resonance(const Args& a) {
    return gi_mol_resonance(a.G, a.N, a.Fn, a.Fe, a.buf, a.buf, a.dtype, nullptr, a.nn_bytes, a.A, a.C, a.H,
                            (const signed char*)a.buf, a.out, a.out, a.out, a.out, a.out, a.edges_out, nullptr);
}

static int kekulize(const Args& a) {
    return gi_mol_kekulize(a.G, a.N, a.Fn, a.Fe, a.buf, a.buf, a.dtype, nullptr, a.nn_bytes, a.A, a.C, a.H,
                           (const signed char*)a.buf, a.out, a.edges_out, nullptr);
}

// the checks the two entry points share
static void common(const char* who, int (*call)(const Args&)) {
    char what[96];
    auto name = [&](const char* s) { std::snprintf(what, sizeof what, "%s: %s", who, s); return what; };
    expect(name("G = 0"), call(Args()), 0);
    { Args a; a.G = -1; expect(name("G < 0"), call(a), GI_EINVAL); }
    { Args a; a.N = 0; expect(name("N = 0"), call(a), GI_EINVAL); }
    { Args a; a.N = GI_MAX_NODES + 1; expect(name("N past the limit"), call(a), GI_EINVAL); }
    { Args a; a.Fe = 0; expect(name("Fe = 0"), call(a), GI_EINVAL); }
    { Args a; a.Fn = GI_ANALYZE_MAX_FN + 1; expect(name("Fn past the limit"), call(a), GI_ELIMIT); }
    { Args a; a.dtype = 7; expect(name("dtype"), call(a), GI_EINVAL); }
    { Args a; a.nn_bytes = 2; expect(name("n_nodes of 2 bytes"), call(a), GI_EINVAL); }
    { Args a; a.A = 0; expect(name("no atom types"), call(a), GI_EINVAL); }
    { Args a; a.A = a.C = 0x7fffffff; expect(name("segments overflow int"), call(a), GI_EINVAL); }
    { Args a; a.H = 1; expect(name("segments past Fn"), call(a), GI_EINVAL); }
    { Args a; a.G = 1; expect(name("no buffers"), call(a), GI_EINVAL); }
}

struct Marks {
    unsigned (*row)[4];
    void mark(int a, int b) { row[a][b >> 5] |= 1u << (b & 31); row[b][a >> 5] |= 1u << (a & 31); }
    bool marked(int a, int b) const { return (row[a][b >> 5] >> (b & 31)) & 1u; }
};

// a ring of n atoms (n even) with a chord between 0 and `chord` (0: none), double bonds (2k, 2k + 1): the delocalised
// bonds counted on the host, the workspaces interleaved with stride `st` as the lanes of a workgroup keep them
static int ring_bonds(int n, int chord, int st) {
    std::vector<unsigned> gp(n * 4, 0u);
    std::vector<unsigned char> mate(n), parent(n * st), base(n * st), queue(n * st);
    auto bond = [&](int a, int b) { gp[a * 4 + (b >> 5)] |= 1u << (b & 31); gp[b * 4 + (a >> 5)] |= 1u << (a & 31); };
    for (int i = 0; i < n; ++i) { bond(i, (i + 1) % n); mate[i] = (unsigned char)(i ^ 1); }
    if (chord) bond(0, chord);
    static unsigned del[128][4];
    for (auto& r : del) for (unsigned& w : r) w = 0u;
    Marks d = {del};
    for (int a = 0; a < n; ++a) res_doubles(gp.data(), n, mate.data(), a, parent.data(), base.data(), queue.data(), st, d);
    for (int u = 0; u < n; ++u) res_singles(gp.data(), n, mate.data(), u, parent.data(), base.data(), queue.data(), st, d);
    int bits = 0;
    for (int i = 0; i < n; ++i) for (int w = 0; w < 4; ++w) bits += __builtin_popcount(del[i][w]);
    return bits / 2;
}

// `match` on a ring of n atoms: 1 and the matching's size, or 0
static int ring_match(int n) {
    std::vector<unsigned> rows(n * 4, 0u);
    std::vector<unsigned char> mate(n), parent(n), base(n), queue(n);
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1) % n;
        rows[i * 4 + (j >> 5)] |= 1u << (j & 31);
        rows[j * 4 + (i >> 5)] |= 1u << (i & 31);
    }
    if (!res_match(rows.data(), n, mate.data(), parent.data(), base.data(), queue.data(), nullptr)) return 0;
    int matched = 0;
    for (int i = 0; i < n; ++i) matched += mate[i] != RES_NONE && mate[mate[i]] == i;
    return matched;
}

int main() {
    common("gi_mol_resonance", resonance);
    common("gi_mol_kekulize", kekulize);
    signed char byte = 0;
    int word[4] = {0, 0, 0, 0};
    { Args a; a.Fe = GI_MAX_GROUPS + 1; expect("resonance: Fe past the limit", resonance(a), GI_EINVAL); }
    { Args a; a.Fe = GI_MAX_GROUPS; expect("resonance: Fe at the limit without the edges", resonance(a), 0); }
    { Args a; a.Fe = GI_MAX_GROUPS; a.edges_out = &byte; expect("resonance: Fe + 1 channels past the limit", resonance(a), GI_ELIMIT); }
    { Args a; a.Fe = GI_MAX_GROUPS - 1; a.edges_out = &byte; expect("resonance: Fe + 1 channels at the limit", resonance(a), 0); }
    { Args a; a.G = 1; a.buf = word; expect("resonance: no outputs", resonance(a), GI_EINVAL); }
    { Args a; a.Fe = GI_MAX_GROUPS; expect("kekulize: Fe + 1 channels past the limit", kekulize(a), GI_ELIMIT); }
    { Args a; a.Fe = GI_MAX_GROUPS - 1; expect("kekulize: Fe + 1 channels at the limit", kekulize(a), 0); }
    { Args a; a.G = 1; a.buf = word; a.out = word; expect("kekulize: no edges", kekulize(a), GI_EINVAL); }
    { Args a; a.G = 1; a.buf = word; a.edges_out = &byte; expect("kekulize: no status", kekulize(a), GI_EINVAL); }
    // the searches, on the host
    expect("benzene", ring_bonds(6, 0, 1), 6);
    expect("a 128-ring, interleaved workspaces", ring_bonds(128, 0, 64), 128);
    expect("naphthalene: the fusion bond too", ring_bonds(10, 5, 3), 11);
    expect("azulene: the fusion bond is not", ring_bonds(10, 6, 3), 10);
    expect("match on an even ring", ring_match(128), 128);
    expect("match on an odd ring", ring_match(7), 0);
    expect("match on one atom", ring_match(1), 0);
    std::printf(failures ? "%d failures\n" : "gi_mol_resonance / gi_mol_kekulize host side: ok\n", failures);
    return failures ? 1 : 0;
}
