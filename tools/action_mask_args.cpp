// The host side of gi_action_mask (argument checks and launch geometry) under a host sanitizer, without a device:
// every call below returns before anything is launched.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igraphinvent_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         graphinvent_amd/csrc/gi_mask.hip tools/action_mask_args.cpp -o /tmp/action_mask_args && /tmp/action_mask_args
#include <climits>
#include <cstdio>

#include "graphinvent_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

struct Args {
    int B = 0, N = 13, Fn = 8, Fe = 3, dtype = GI_DTYPE_F32, nn_bytes = 1, n_groups = 2;
    int group[GI_GROW_MAX_GROUPS + 1] = {5, 3};
    const int* groups = group;
    int T = 5, C = 3, H = 0, valence = 1, allow_empty = 0, ld = 13 * 45 + 13 * 3 + 1, ld2 = 0;
    const void* state = nullptr;
    const float* logits = nullptr;
    float* masked = nullptr;
    const float* logits2 = nullptr;
    float* masked2 = nullptr;
    int* out = nullptr;
};

static int call(const Args& a) {
    return gi_action_mask(a.B, a.N, a.Fn, a.Fe, a.state, a.state, a.dtype, a.state, a.nn_bytes, a.n_groups, a.groups, a.T,
                          a.C, a.H, (const unsigned short*)a.state, (const signed char*)a.state,
                          (const signed char*)a.state, a.valence, a.allow_empty, a.logits, a.ld, a.masked, a.ld,
                          a.logits2, a.ld2, a.masked2, a.ld2, a.out, a.out, nullptr, nullptr, nullptr);
}

int main() {
    Args ok;
    expect("B = 0", call(ok), 0);
    { Args a; a.B = -1; expect("B < 0", call(a), GI_EINVAL); }
    { Args a; a.N = 0; expect("N = 0", call(a), GI_EINVAL); }
    { Args a; a.N = GI_MAX_NODES + 1; expect("N past the limit", call(a), GI_EINVAL); }
    { Args a; a.Fe = GI_MAX_GROUPS + 1; expect("Fe past the limit", call(a), GI_EINVAL); }
    { Args a; a.Fn = GI_ANALYZE_MAX_FN + 1; expect("Fn past the limit", call(a), GI_ELIMIT); }
    { Args a; a.dtype = 7; expect("dtype", call(a), GI_EINVAL); }
    { Args a; a.nn_bytes = 2; expect("n_nodes of 2 bytes", call(a), GI_EINVAL); }
    { Args a; a.T = 0; expect("no atom types", call(a), GI_EINVAL); }
    { Args a; a.T = a.C = 0x7fffffff; expect("segments overflow int", call(a), GI_EINVAL); }
    { Args a; a.H = -1; expect("n_imp_h < 0", call(a), GI_EINVAL); }
    { Args a; a.valence = 2; expect("valence = 2", call(a), GI_EINVAL); }
    { Args a; a.allow_empty = -1; expect("allow_empty = -1", call(a), GI_EINVAL); }
    { Args a; a.groups = nullptr; expect("no groups", call(a), GI_EINVAL); }
    { Args a; a.n_groups = 1; expect("one group", call(a), GI_EINVAL); }
    { Args a; a.n_groups = GI_GROW_MAX_GROUPS + 1; expect("too many groups", call(a), GI_EINVAL); }
    { Args a; a.group[1] = 0; expect("an empty group", call(a), GI_EINVAL); }
    { Args a; a.group[0] = 4; a.group[1] = 4; expect("groups are not the segments", call(a), GI_EINVAL); }
    { Args a; a.Fn = 9; expect("groups do not tile Fn", call(a), GI_EINVAL); }
    { Args a; a.n_groups = 3; a.group[2] = 4; a.Fn = 12; a.H = 3; expect("H is not group 2", call(a), GI_EINVAL); }
    { Args a; a.n_groups = 3; a.group[2] = 4; a.Fn = 12; a.H = 4; a.ld = 13 * 183 + 1; expect("with H", call(a), 0); }
    { Args a; a.ld -= 1; expect("pitch below W", call(a), GI_EINVAL); }
    {
        Args a;                                              // prod(group) * Fe past INT_MAX
        a.n_groups = 8;
        for (int k = 0; k < 7; ++k) a.group[k] = 8;
        a.group[7] = 456;
        a.Fn = 512;
        a.T = a.C = 8;
        a.ld = INT_MAX;
        expect("A overflows int", call(a), GI_ELIMIT);
    }
    {
        Args a;                                              // W = N A + N Fe + 1 past INT_MAX
        a.N = 128;
        a.n_groups = 4;
        a.group[0] = a.group[1] = a.group[2] = a.group[3] = 100;
        a.Fn = 400;
        a.T = a.C = 100;
        a.ld = INT_MAX;
        expect("W overflows int", call(a), GI_ELIMIT);
    }
    {
        Args a;
        a.n_groups = 3;
        a.group[0] = a.group[1] = a.group[2] = 70;
        a.Fn = 210;
        a.T = a.C = a.H = 70;
        a.ld = INT_MAX;
        expect("too many (type, charge, H) combinations", call(a), GI_ELIMIT);
    }
    float rows[8];
    int word = 0;
    {
        Args a;
        a.B = 1;
        expect("no buffers", call(a), GI_EINVAL);
        a.state = &word;
        a.out = &word;
        a.logits = rows;
        a.masked = rows;
        expect("masked is the logits", call(a), GI_EINVAL);
        a.masked = rows + 4;
        a.logits2 = rows;
        expect("a second matrix without its copy", call(a), GI_EINVAL);
        a.masked2 = rows + 4;
        a.ld2 = a.ld;
        expect("both copies in one place", call(a), GI_EINVAL);
        a.masked2 = rows + 2;
        a.ld2 = a.ld - 1;
        expect("second pitch below W", call(a), GI_EINVAL);
    }
    expect("stats: B < 0", gi_action_mask_stats(-1, rows, nullptr, &word, rows, nullptr), GI_EINVAL);
    expect("stats: B = 0", gi_action_mask_stats(0, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
    expect("stats: no buffers", gi_action_mask_stats(1, nullptr, nullptr, &word, rows, nullptr), GI_EINVAL);
    std::printf(failures ? "%d failures\n" : "gi_action_mask argument checks: ok\n", failures);
    return failures ? 1 : 0;
}
