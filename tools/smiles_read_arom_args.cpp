// The host side of gi_smiles_read_arom (argument checks and launch geometry) under a host sanitizer, without a device:
// every call below returns before anything is launched.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igraphinvent_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         graphinvent_amd/csrc/gi_smiles_read.hip tools/smiles_read_arom_args.cpp -o /tmp/smiles_read_arom_args && \
//   /tmp/smiles_read_arom_args
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

static int call(int aromatic, int G, int N, int Fn, int Fe, int max_len, int A, int C, int H, int none, int drop) {
    return gi_smiles_read_arom(G, N, Fn, Fe, nullptr, nullptr, max_len, A, C, H, nullptr, nullptr, nullptr, nullptr,
                               nullptr, none, drop, aromatic, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int main() {
    for (int aromatic = 0; aromatic < 2; ++aromatic) {      // both instantiations share every check
        expect("G = 0", call(aromatic, 0, 13, 12, 3, 160, 5, 3, 4, 0, 0), 0);
        expect("G = 0 at every limit",
               call(aromatic, 0, GI_MAX_NODES, GI_ANALYZE_MAX_FN, GI_MAX_GROUPS, GI_SMI_MAX_LEN, 5, 3, 0, 503, 1), 0);
        expect("no buffers", call(aromatic, 1, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("G < 0", call(aromatic, -1, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("N = 0", call(aromatic, 0, 0, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("N past the limit", call(aromatic, 0, GI_MAX_NODES + 1, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("Fe = 0", call(aromatic, 0, 13, 12, 0, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("Fe past the limit", call(aromatic, 0, 13, 12, GI_MAX_GROUPS + 1, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("Fn past the limit", call(aromatic, 0, 13, GI_ANALYZE_MAX_FN + 1, 3, 160, 5, 3, 4, 0, 0), GI_ELIMIT);
        expect("segments wider than Fn", call(aromatic, 0, 13, 11, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("segments overflow int", call(aromatic, 0, 13, 12, 3, 160, 0x7fffffff, 0x7fffffff, 4, 0, 0), GI_EINVAL);
        expect("none_chirality past the rest", call(aromatic, 0, 13, 14, 3, 160, 5, 3, 4, 2, 0), GI_EINVAL);
        expect("drop_stereo = 2", call(aromatic, 0, 13, 12, 3, 160, 5, 3, 4, 0, 2), GI_EINVAL);
        expect("max_len not a multiple of 16", call(aromatic, 0, 13, 12, 3, 24, 5, 3, 4, 0, 0), GI_EINVAL);
        expect("max_len past the limit", call(aromatic, 0, 13, 12, 3, GI_SMI_MAX_LEN + 16, 5, 3, 4, 0, 0), GI_ELIMIT);
    }
    expect("aromatic = 2", call(2, 0, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("aromatic = -1", call(-1, 0, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("aromatic = 2 with buffers missing", call(2, 1, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    expect("aromatic = INT_MIN", call(static_cast<int>(0x80000000u), 0, 13, 12, 3, 160, 5, 3, 4, 0, 0), GI_EINVAL);
    unsigned char text[48];
    int word = 0;
    unsigned short allowed = 0;
    signed char table = 0;
    expect("text not 16-byte aligned",
           gi_smiles_read_arom(1, 1, 2, 1, text + (16 - (reinterpret_cast<uintptr_t>(text) & 15)) % 16 + 1, nullptr, 16, 1,
                               1, 0, &allowed, &table, nullptr, &table, text, 0, 0, 1, &table, &table, &word, &word, &word,
                               nullptr),
           GI_EINVAL);
    expect("the old entry point, unchanged",
           gi_smiles_read(0, 13, 12, 3, nullptr, nullptr, 160, 5, 3, 4, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
    std::printf(failures ? "%d failures\n" : "gi_smiles_read_arom argument checks: ok\n", failures);
    return failures ? 1 : 0;
}
