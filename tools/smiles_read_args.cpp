// The host side of gi_smiles_read (argument checks and launch geometry) under a host sanitizer, without a device:
// every call below returns before anything is launched.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igraphinvent_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         graphinvent_amd/csrc/gi_smiles_read.hip tools/smiles_read_args.cpp -o /tmp/smiles_read_args && /tmp/smiles_read_args
#include <cstdint>
#include <cstdio>

#include "graphinvent_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

static int call(int G, int N, int Fn, int Fe, int max_len, int A, int C, int H, int none, int drop) {
    return gi_smiles_read(G, N, Fn, Fe, nullptr, nullptr, max_len, A, C, H, nullptr, nullptr, nullptr, nullptr, nullptr,
                          none, drop, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int main() {
    expect("G = 0", call(0, 13, 12, 3, 160, 5, 3, 4, 0, 0), 0);
    expect("G = 0 at every limit", call(0, GI_MAX_NODES, GI_ANALYZE_MAX_FN, GI_MAX_GROUPS, GI_SMI_MAX_LEN, 5, 3, 0, 503, 1), 0);
    expect("no buffers", call(1, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("G < 0", call(-1, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("N = 0", call(0, 0, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("N past the limit", call(0, GI_MAX_NODES + 1, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("Fe = 0", call(0, 13, 12, 0, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("Fe past the limit", call(0, 13, 12, GI_MAX_GROUPS + 1, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("Fn past the limit", call(0, 13, GI_ANALYZE_MAX_FN + 1, 3, 160, 5, 3, 4, 0, 0), GI_ELIMIT);
    expect("segments wider than Fn", call(0, 13, 11, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("segments overflow int", call(0, 13, 12, 3, 160, 0x7fffffff, 0x7fffffff, 4, 0, 0), GI_EINVAL);
    expect("no atom types", call(0, 13, 12, 3, 160, 0, 3, 4, 0, 0), GI_EINVAL);
    expect("n_imp_h < 0", call(0, 13, 12, 3, 160, 5, 3, -1, 0, 0), GI_EINVAL);
    expect("none_chirality < 0", call(0, 13, 12, 3, 160, 5, 3, 4, -1, 0), GI_EINVAL);
    expect("none_chirality past the rest", call(0, 13, 14, 3, 160, 5, 3, 4, 2, 0), GI_EINVAL);
    expect("none_chirality inside the rest", call(0, 13, 14, 3, 160, 5, 3, 4, 1, 0), 0);
    expect("drop_stereo = 2", call(0, 13, 12, 3, 160, 5, 3, 4, 0, 2), GI_EINVAL);
    expect("max_len = 0", call(0, 13, 12, 3, 0, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("max_len not a multiple of 16", call(0, 13, 12, 3, 24, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("max_len past the limit", call(0, 13, 12, 3, GI_SMI_MAX_LEN + 16, 5, 3, 4, 0, 0), GI_ELIMIT);
    unsigned char text[48];
    int word = 0;
    unsigned short allowed = 0;
    signed char table = 0;
    expect("text not 16-byte aligned",
           gi_smiles_read(1, 1, 2, 1, text + (16 - (reinterpret_cast<uintptr_t>(text) & 15)) % 16 + 1, nullptr, 16, 1, 1, 0,
                          &allowed, &table, nullptr, &table, text, 0, 0, &table, &table, &word, &word, &word, nullptr),
           GI_EINVAL);
    std::printf(failures ? "%d failures\n" : "gi_smiles_read argument checks: ok\n", failures);
    return failures ? 1 : 0;
}
