// The host side of gi_mol_substructure (argument checks and the pattern table's checks) under a host sanitizer, without
// a device: every call below returns before anything is launched.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igraphinvent_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         graphinvent_amd/csrc/gi_substructure.hip tools/substructure_args.cpp -o /tmp/substructure_args && /tmp/substructure_args
#include <cstdio>
#include <vector>

#include "graphinvent_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

// One pattern, a triangle of "any" atoms with bond type 0 (plan 0, 1, 2; the ring closes from position 2 to 1), under
// A = 5 types, C = 3 charges, Fe = 3: header 8, record 4 + 3 rows of 12 + 4 back bonds.
static std::vector<int> triangle() {
    std::vector<int> t(8 + 4 + 3 * 12 + 4, 0);
    const int hdr[8] = {1, 3, 5, 3, 3, 1, 1, 4};
    for (int i = 0; i < 8; ++i) t[i] = hdr[i];
    t[8] = 3;
    for (int k = 0; k < 3; ++k) {
        int* row = &t[12 + 12 * k];
        row[0] = 0;                                          // parent
        row[1] = k ? 1 : 0;                                  // parent bond mask
        row[2] = 0;
        row[3] = k == 2 ? 1 : 0;                             // back bonds
        row[4] = k;
        row[5] = row[6] = -1;
        row[8] = 0x1f;
        row[9] = 0x7;
    }
    t[12 + 36] = 1 | (1 << 8);                               // position 2 -> position 1, type 0
    return t;
}

struct Args {
    int G = 0, N = 13, Fn = 8, Fe = 3, dtype = GI_DTYPE_I8, nn_bytes = 1, A = 5, C = 3, H = 0, max_steps = 4096;
    std::vector<int> table = triangle();
    long long words = -1;
    const void* buf = nullptr;
    int* out = nullptr;
    const int* dev_table = nullptr;
    bool host_table = true;
};

static int call(const Args& a) {
    return gi_mol_substructure(a.G, a.N, a.Fn, a.Fe, a.buf, a.buf, a.dtype, nullptr, a.nn_bytes, a.A, a.C, a.H,
                               (const unsigned short*)a.buf, (const signed char*)a.buf,
                               a.host_table ? a.table.data() : nullptr, a.dev_table,
                               a.words < 0 ? (long long)a.table.size() : a.words, nullptr, a.max_steps, a.out, a.out, a.out,
                               a.out, a.out, a.out, nullptr);
}

static int with(int offset, int value) {
    Args a;
    a.table[offset] = value;
    return call(a);
}

int main() {
    expect("G = 0", call(Args()), 0);
    { Args a; a.host_table = false; expect("G = 0 without a table", call(a), 0); }
    { Args a; a.G = -1; expect("G < 0", call(a), GI_EINVAL); }
    { Args a; a.N = 0; expect("N = 0", call(a), GI_EINVAL); }
    { Args a; a.N = GI_MAX_NODES + 1; expect("N past the limit", call(a), GI_EINVAL); }
    { Args a; a.Fe = GI_MAX_GROUPS + 1; expect("Fe past the limit", call(a), GI_EINVAL); }
    { Args a; a.Fn = GI_ANALYZE_MAX_FN + 1; expect("Fn past the limit", call(a), GI_ELIMIT); }
    { Args a; a.dtype = 7; expect("dtype", call(a), GI_EINVAL); }
    { Args a; a.nn_bytes = 2; expect("n_nodes of 2 bytes", call(a), GI_EINVAL); }
    { Args a; a.A = 0; expect("no atom types", call(a), GI_EINVAL); }
    { Args a; a.A = a.C = 0x7fffffff; expect("segments overflow int", call(a), GI_EINVAL); }
    { Args a; a.H = 1; expect("segments past Fn", call(a), GI_EINVAL); }
    { Args a; a.max_steps = 0; expect("max_steps = 0", call(a), GI_EINVAL); }
    { Args a; a.max_steps = GI_SUB_MAX_STEPS + 1; expect("max_steps past the limit", call(a), GI_ELIMIT); }
    { Args a; a.max_steps = GI_SUB_MAX_STEPS; expect("max_steps at the limit", call(a), 0); }
    // the table's header
    { Args a; a.words = 7; expect("a table shorter than its header", call(a), GI_EINVAL); }
    { Args a; a.words = (long long)a.table.size() - 1; expect("a table shorter than it says", call(a), GI_EINVAL); }
    { Args a; a.table.push_back(0); expect("a table longer than it says", call(a), GI_EINVAL); }
    expect("P = 0", with(0, 0), GI_EINVAL);
    expect("P past the limit", with(0, GI_SUB_MAX_PATTERNS + 1), GI_ELIMIT);
    expect("P = 2^31 - 1 in a table of one", with(0, 0x7fffffff), GI_ELIMIT);
    expect("P = 2 in a table of one", with(0, 2), GI_EINVAL);
    expect("Np_max = 0", with(1, 0), GI_EINVAL);
    expect("Np_max past the limit", with(1, GI_SUB_MAX_ATOMS + 1), GI_ELIMIT);
    expect("other atom types", with(2, 6), GI_EINVAL);
    expect("other charges", with(3, 2), GI_EINVAL);
    expect("other bond types", with(4, 4), GI_EINVAL);
    expect("TW", with(5, 2), GI_EINVAL);
    expect("CW", with(6, 0), GI_EINVAL);
    expect("B not a multiple of 4", with(7, 3), GI_EINVAL);
    expect("B < 0", with(7, -4), GI_EINVAL);
    expect("B past Np (Np - 1) / 2", with(7, 8), GI_EINVAL);
    // the plan
    expect("Np = 0", with(8, 0), GI_EINVAL);
    expect("Np past Np_max", with(8, 4), GI_EINVAL);
    expect("position 0 with a parent", with(12, 1), GI_EINVAL);
    expect("position 0 with a parent bond", with(13, 1), GI_EINVAL);
    expect("a parent that is the child", with(24, 1), GI_EINVAL);
    expect("a parent after the child", with(36, 2), GI_EINVAL);
    expect("a negative parent", with(36, -1), GI_EINVAL);
    expect("a parent bond without types", with(25, 0), GI_EINVAL);
    expect("a parent bond of a type past Fe", with(25, 8), GI_EINVAL);
    expect("an atom twice", with(28, 0), GI_EINVAL);
    expect("an atom past Np", with(40, 3), GI_EINVAL);
    expect("a negative atom", with(40, -1), GI_EINVAL);
    expect("back bonds from before the list", with(38, -1), GI_EINVAL);
    expect("back bonds past the list", with(39, 5), GI_EINVAL);
    expect("a negative number of back bonds", with(39, -1), GI_EINVAL);
    expect("first + count overflows", with(38, 0x7fffffff), GI_EINVAL);
    expect("a back bond to a later position", with(48, 2 | (1 << 8)), GI_EINVAL);
    expect("a back bond to the parent", with(48, 0 | (1 << 8)), GI_EINVAL);
    expect("a back bond without types", with(48, 1), GI_EINVAL);
    expect("a back bond of a type past Fe", with(48, 1 | (8 << 8)), GI_EINVAL);
    expect("a negative back bond", with(48, -1), GI_EINVAL);
    expect("degree past N - 1", with(17, GI_MAX_NODES), GI_EINVAL);
    expect("degree below -1", with(17, -2), GI_EINVAL);
    expect("min_h past 15", with(18, 16), GI_EINVAL);
    expect("a type bit past A", with(20, 0x3f), GI_EINVAL);
    expect("a charge bit past C", with(21, 0xf), GI_EINVAL);
    expect("a degree, some hydrogens, one type", [] { Args a; a.table[17] = 3; a.table[18] = 2; a.table[20] = 4; return call(a); }(), 0);
    // buffers
    int word[4] = {0, 0, 0, 0};
    alignas(16) int aligned[8] = {0};
    {
        Args a;
        a.G = 1;
        expect("no buffers", call(a), GI_EINVAL);
        a.buf = word;
        a.out = word;
        expect("no device table", call(a), GI_EINVAL);
        a.dev_table = aligned + 1;
        expect("a device table off its 16 bytes", call(a), GI_EINVAL);
        a.dev_table = aligned;
        a.host_table = false;
        expect("no host table", call(a), GI_EINVAL);
    }
    std::printf(failures ? "%d failures\n" : "gi_mol_substructure argument checks: ok\n", failures);
    return failures ? 1 : 0;
}
