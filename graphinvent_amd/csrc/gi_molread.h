// The molecule reader shared by gi_canon.hip and gi_valence.hip (one 256-lane workgroup per molecule): every byte of a
// [G, N, Fn] / [G, N, N, Fe] tensor of fp32 or int8 is read once, in 16-byte pieces between ragged ends, at any element
// alignment.  (gi_analyze.hip keeps a reader of its own: it hands the VALUE of every entry to its statistics.)
#pragma once
#include "gi_common.h"

constexpr int GI_MOL_NT = 256;                               // lanes of a workgroup that reads a molecule

__device__ __forceinline__ bool gi_is01(float x) { return x == 0.f || x == 1.f; }
__device__ __forceinline__ bool gi_is01(signed char x) { return x == 0 || x == 1; }

__device__ __forceinline__ long long gi_load_count(const void* p, int bytes, long long g) {
    return bytes == 1 ? (long long)((const signed char*)p)[g] : bytes == 4 ? (long long)((const int*)p)[g]
                                                                           : ((const long long*)p)[g];
}

// f(offset, is the value 1) for every non-zero element of p[0, len): whole 16-byte granules of the ADDRESS range are one
// load each, a ragged first or last granule is read element by element; nothing outside p[0, len) is touched
template <typename T, class F>
__device__ __forceinline__ void gi_for_each_nonzero(const T* p, int len, int tid, F f) {
    constexpr int E = 16 / (int)sizeof(T);
    const int shift = (int)(((uintptr_t)p & 15) / sizeof(T));
    const int P = (shift + len + E - 1) / E;
    for (int q = tid; q < P; q += GI_MOL_NT) {
        const int lo = q * E - shift;
        const int a = max(lo, 0), b = min(lo + E, len);
        T v[E];
        if (b - a == E) {
            const uint4 w = *reinterpret_cast<const uint4*>(p + a);
            if ((w.x | w.y | w.z | w.w) == 0) continue;     // molecules are mostly zeros (+0.f is all zero bits)
            __builtin_memcpy(v, &w, 16);
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = k < b - a ? p[a + k] : (T)0;
        }
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (k < b - a && !(v[k] == (T)0)) f(a + k, gi_is01(v[k]));
    }
}

// bits [0, k) set, 0 <= k <= 128, as four 32-bit words
__device__ __forceinline__ unsigned gi_below_word(int k, int w) {
    const int r = k - 32 * w;
    return r <= 0 ? 0u : r >= 32 ? ~0u : (1u << r) - 1u;
}
