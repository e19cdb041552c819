"""CPU: the launch plan of the GEMM kernel family (graphinvent_amd/csrc/gi_gemm_plan.h, host part).

A stand-alone C++ program includes the header's host part and the five capability rows as the kernel files state them
(the `constexpr GiGemmCaps ..._CAPS` initialisers are lifted from the .hip files), builds the plan of every case below
and prints one line per case: rc, n, total, start[], gx[], gy[], remap, epi, flags[] (what the kernels get).  The
expected values were written from the launchers as they were before the plan existed (gi_gemm_batch + validate,
gi_gemm_bf3_launch, gi_x2n_launch, gi_b3v_launch, gi_b3p_launch), by reading them; where two launchers answered one
malformed descriptor differently, each row keeps its own answer:
  * a missing bias / act pointer: the fp32 launcher never looked (rc 0), the others answer GI_EINVAL;
  * ones_col on a contiguous B: the 16-deep bf16x3 launcher and x2n never read the field, the others answer GI_EINVAL;
  * an odd leading dimension of a major operand: b3v reads column pairs (GI_EINVAL), b3p single columns (accepted);
  * a weight-gradient launch of 16+ tiles: b3p always walks it slab by slab, b3v only its fp16x2 form.
Unified: a contiguous operand with K < 4 and K <= ld < 4 is GI_EINVAL everywhere (b3v said GI_ELIMIT), and more than
0x3fffffff tiles is GI_ELIMIT in every row (the 16-deep launcher and x2n used to add the tiles up unchecked).
Built with -fsanitize=address,undefined where that links (a stand-alone program: no preload involved)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphinvent_amd", "csrc")
ROWS = {"tiles": ("gi_gemm.hip", "TILES_CAPS"), "bf3": ("gi_gemm_bf3.hip", "B3_CAPS"), "x2n": ("gi_gemm_x2n.hip", "XN_CAPS"),
        "b3v": ("gi_gemm_b3v.hip", "GV_CAPS"), "b3p": ("gi_gemm_b3p.hip", "GP_CAPS")}
EINVAL, ELIMIT = -1, -2
BIAS, SELU, DSELU, ACCUM, SPLITK, MULACT, BF3, BF3A, BF3B, X2, T128 = 1, 2, 4, 8, 16, 64, 128, 256, 512, 1024, 2048
# the routing bits a well-formed forward problem of each row carries
ROUTE = {"tiles": 0, "bf3": BF3 | BF3B, "x2n": BF3 | BF3B | X2, "b3v": BF3 | BF3B, "b3p": BF3 | BF3B}
TILE = {"tiles": (64, 64), "bf3": (128, 128), "x2n": (128, 128), "b3v": (128, 128), "b3p": (128, 256)}

PROLOGUE = r"""
#include <stdio.h>
#include "gi_gemm_plan.h"
static float buf[64] __attribute__((aligned(16)));
static int ibuf[16] = {0, 100, 200, 300, 400, 500, 600, 700, 800, 900};
// a well-formed problem: lay 0 = contig/contig, 1 = contig/major, 2 = major/major (stored columns padded to 4)
static gi_gemm_params mk(int lay, int M, int N, int K, int flags) {
    gi_gemm_params p;
    memset(&p, 0, sizeof(p));
    p.A = p.B = p.bias = p.act = buf; p.C = buf; p.a_amax = p.b_amax = buf;
    p.M = M; p.N = N; p.K = K; p.flags = flags;
    p.a_major = lay == 2; p.b_major = lay >= 1;
    p.lda = p.a_major ? ((M + 3) & ~3) : ((K + 3) & ~3);
    p.ldb = p.b_major ? ((N + 3) & ~3) : ((K + 3) & ~3);
    p.ldc = p.ldact = (N + 3) & ~3;
    p.tm = p.tn = 1; p.nsplit = 1; p.ones_col = -1;
    p.c_split_stride = (long long)M * p.ldc;
    return p;
}
static void run(const char* name, const GiGemmCaps& caps, const gi_gemm_params* p, int n) {
    GiGemmBatch b;
    double flops;
    int epi;
    const int rc = gi_plan_build(p, n, caps, &b, &flops, &epi);
    printf("%s %d", name, rc);
    if (rc == 0) {
        printf(" %d %d", b.n, b.total);
        for (int i = 0; i <= b.n; ++i) printf("%c%d", i ? ',' : ' ', b.start[i]);
        for (int i = 0; i < b.n; ++i) printf("%c%d", i ? ',' : ' ', b.gx[i]);
        for (int i = 0; i < b.n; ++i) printf("%c%d", i ? ',' : ' ', b.gy[i]);
        printf(" %d %d", b.remap, epi);
        for (int i = 0; i < b.n; ++i) printf("%c%d", i ? ',' : ' ', b.p[i].flags);
    }
    printf("\n");
}
"""


def _caps_source():
    """The five rows and the tile constants their initialisers name, as the kernel files state them."""
    out = []
    for row, (fname, sym) in ROWS.items():
        text = open(os.path.join(CSRC, fname)).read()
        for a, av, b, bv in re.findall(r"constexpr int (\w+_BM) = (\d+), (\w+_BN) = (\d+)", text):
            out.append(f"constexpr int {a} = {av}, {b} = {bv};")
        m = re.search(r"constexpr GiGemmCaps %s = \{.*?\};" % sym, text, flags=re.S)
        assert m, (fname, sym)
        out.append("static " + m.group(0) if not m.group(0).startswith("static") else m.group(0))
    return "\n".join(out)


def _ok(n, total, start, gx, gy, remap, epi, flags):
    j = lambda v: ",".join(str(x) for x in v)
    return f"0 {n} {total} {j(start)} {j(gx)} {j(gy)} {remap} {epi} {j(flags)}"


def _cases():
    """[(name, row, C++ statements filling `gi_gemm_params p[8]; int n;`, expected line without the name)]"""
    cases = []

    def add(name, row, body, expect):
        cases.append((f"{row}.{name}", row, body, str(expect)))

    for row in ROWS:
        R, (bm, bn), fwd = ROUTE[row], TILE[row], ROUTE[row] | BIAS | SELU
        cd = lambda a, b: (a + b - 1) // b
        own = row == "tiles"                                   # epilogue: 1 = the layout's own / 0 = run-time flags
        # ---- an accepted launch of three problems, the middle one without rows
        three = (f"p[0] = mk(0, 300, 200, 36, {fwd}); p[1] = mk(0, 0, 200, 36, {fwd}); p[2] = mk(0, 130, 257, 36, {fwd}); n = 3;")
        t0, t2 = cd(200, bn) * cd(300, bm), cd(257, bn) * cd(130, bm)
        add("three", row, three, _ok(2, t0 + t2, [0, t0, t0 + t2], [cd(200, bn), cd(257, bn)], [cd(300, bm), cd(130, bm)], 0, 1,
                                     [BIAS | SELU] * 2))
        # ---- every-problem-or-none rules
        add("mix_x2", row, three + f" p[2].flags ^= {X2};", EINVAL)           # (fp32: an unknown flag)
        add("mix_layout", row, three + " p[2].b_major = 1;", EINVAL)
        if row == "tiles":
            add("mix_tile", row, three + " p[2].tn = 2;", EINVAL)
            add("bad_tile", row, three + " p[0].tm = p[1].tm = p[2].tm = 2;", EINVAL)
            add("routing_bit_t128", row, three + f" p[0].flags |= {T128};", EINVAL)      # what keeps GI_TILES_* internal
            add("routing_bit_32", row, three + " p[0].flags |= 32;", EINVAL)
        if row == "bf3":
            add("mix_bf3a", row, three + f" p[2].flags |= {BF3A};", EINVAL)
            add("mix_bf3b", row, three + f" p[2].flags &= ~{BF3B};", EINVAL)
            add("image_b_unaligned", row, f"p[0] = mk(0, 300, 200, 36, {BF3}); p[0].B = buf + 1; n = 1;", EINVAL)
            add("image_b", row, f"p[0] = mk(0, 300, 200, 36, {BF3}); n = 1;", _ok(1, 6, [0, 6], [2], [3], 0, 0, [0]))
            add("image_a_x2", row, f"p[0] = mk(0, 300, 200, 36, {BF3 | BF3A | BF3B | X2}); n = 1;", EINVAL)
        # a gathered B: fp16x2 weight-gradient slabs only (b3v, b3p: every problem or none); fp32: any major B
        wg = X2 if row in ("b3v", "b3p") else 0
        slabs = (f"p[0] = mk(2, 129, 200, 4096, {(R & ~BF3B) | wg | SPLITK}); p[0].nsplit = 2; p[0].lda = 130; p[1] = p[0]; n = 2;")
        mm_ok = row in ("tiles", "b3v", "b3p")
        mm_tiles = 2 * cd(200, bn) * cd(129, bm)
        mm_epi = 1 if own else 3
        mm_line = _ok(2, 2 * mm_tiles, [0, mm_tiles, 2 * mm_tiles], [cd(200, bn)] * 2, [cd(129, bm)] * 2,
                      1 if (row in ("b3v", "b3p") and 2 * mm_tiles >= 16) else 0, mm_epi, [SPLITK] * 2)
        add("slabs", row, slabs, mm_line if mm_ok else EINVAL)
        add("mix_bidx", row, slabs + " p[1].b_idx = ibuf;", mm_line if row == "tiles" else EINVAL)
        add("bidx_all", row, slabs + " p[0].b_idx = p[1].b_idx = ibuf;", mm_line if mm_ok else EINVAL)
        add("bidx_contig_b", row, three + " p[0].b_idx = ibuf;", EINVAL)
        if row in ("b3v", "b3p"):
            add("bidx_bf16x3", row, slabs + f" p[0].flags &= ~{X2}; p[1].flags &= ~{X2}; p[0].b_idx = p[1].b_idx = ibuf;", EINVAL)
        add("a_idx", row, three + " p[0].a_idx = ibuf;", _ok(2, 35, [0, 20, 35], [4, 5], [5, 3], 0, 1, [3, 3]) if own else EINVAL)
        add("k_dev", row, three + " p[0].k_dev = ibuf;", _ok(2, 35, [0, 20, 35], [4, 5], [5, 3], 0, 1, [3, 3]) if own else EINVAL)
        # ---- malformed descriptors
        dgrad = f"p[0] = mk(1, 300, 200, 36, {(R & ~BF3B) | DSELU}); n = 1;"
        add("ones_col_not_last", row, dgrad + " p[0].ones_col = 198;", EINVAL)
        # (the 16-deep kernel's launcher and x2n never read ones_col: a zeroed descriptor, ones_col = 0, is a forward problem)
        add("ones_col_contig_b", row, three + " p[0].ones_col = 199;", EINVAL if row not in ("bf3", "x2n") else
            _ok(2, t0 + t2, [0, t0, t0 + t2], [cd(200, bn), cd(257, bn)], [cd(300, bm), cd(130, bm)], 0, 1, [3, 3]))
        add("ones_col_zeroed", row, three + " for (int i = 0; i < 3; ++i) p[i].ones_col = 0;", EINVAL if row not in ("bf3", "x2n") else
            _ok(2, t0 + t2, [0, t0, t0 + t2], [cd(200, bn), cd(257, bn)], [cd(300, bm), cd(130, bm)], 0, 1, [3, 3]))
        add("nsplit_without_splitk", row, three + " p[2].nsplit = 2;", EINVAL)
        add("gsplit_zero", row, slabs + " p[1].ngroups = 2; p[1].grp_off = ibuf; p[1].gsplit[0] = 1; p[1].gsplit[1] = 0;"
            " p[1].Cg[0] = p[1].Cg[1] = buf;", EINVAL)
        add("groups_without_grp_off", row, slabs + " p[1].ngroups = 2; p[1].gsplit[0] = p[1].gsplit[1] = 1;", EINVAL)
        line3 = _ok(2, 35, [0, 20, 35], [4, 5], [5, 3], 0, 1, [3, 3])
        add("no_bias", row, three + " p[2].bias = nullptr;", line3 if own else EINVAL)
        add("no_act", row, f"p[0] = mk(0, 300, 200, 36, {R | DSELU}); p[0].act = nullptr; n = 1;",
            _ok(1, 20, [0, 20], [4], [5], 0, 0, [DSELU]) if own else EINVAL)
        if row != "tiles":
            add("no_amax", row, three + f" for (int i = 0; i < 3; ++i) p[i].flags |= {X2}; p[1].b_amax = nullptr;", EINVAL)
            add("no_a", row, three + " p[1].A = nullptr;", EINVAL)
            add("no_c", row, three + " p[1].C = nullptr;", EINVAL)
        add("splitk_bounded", row, slabs + " p[0].m_dev = ibuf;", EINVAL)
        add("k_lt_4_unpadded", row, f"p[0] = mk(0, 300, 200, 2, {fwd}); p[0].lda = 2; n = 1;", EINVAL)
        add("k_lt_4_unpadded_b", row, f"p[0] = mk(0, 300, 200, 2, {fwd}); p[0].ldb = 3; n = 1;", EINVAL)
        add("unknown_flag", row, three + " p[0].flags |= 4096;", EINVAL)
        if row != "tiles":
            add("lda_lt_k", row, three + " p[2].lda = 35;", EINVAL)
        # ---- 32-bit offsets: M * lda just below and just above 0xffffffff / 4 (1023 / 1024 rows of 2^20 floats)
        big = lambda M: f"p[0] = mk(0, {M}, 200, 36, {fwd}); p[0].lda = 1 << 20; n = 1;"
        tb = cd(200, bn) * cd(1023, bm)
        add("offset_below", row, big(1023), _ok(1, tb, [0, tb], [cd(200, bn)], [cd(1023, bm)], 0, 1, [3]))
        add("offset_above", row, big(1024), ELIMIT)
        add("offset_above_b", row, f"p[0] = mk(0, 300, 1024, 36, {fwd}); p[0].ldb = 1 << 20; n = 1;", ELIMIT)
        # ---- major operands with an odd leading dimension: b3v reads column pairs
        odd = f"p[0] = mk(2, 129, 200, 4096, {(R & ~BF3B) | SPLITK}); p[0].nsplit = 2; p[0].lda = 129; n = 1;"
        if mm_ok:
            add("odd_lda_major", row, odd, EINVAL if row == "b3v" else
                _ok(1, mm_tiles, [0, mm_tiles], [cd(200, bn)], [cd(129, bm)], 0, mm_epi, [SPLITK]))
            add("even_lda_major", row, odd + " p[0].lda = 130;",
                _ok(1, mm_tiles, [0, mm_tiles], [cd(200, bn)], [cd(129, bm)], 0, mm_epi, [SPLITK]))
            add("short_lda_major", row, odd + " p[0].lda = 128;", EINVAL if row != "tiles" else      # (fp32: never checked)
                _ok(1, mm_tiles, [0, mm_tiles], [cd(200, bn)], [cd(129, bm)], 0, mm_epi, [SPLITK]))
        # ---- tile order: the row rule on both sides of its threshold, with and without m_dev
        if row == "tiles":
            lo, hi, thr = (71 * 64, 19 * 64), (50 * 64, 27 * 64), 1350          # 1349 / 1350 workgroups
        else:
            lo, hi, thr = (73 * bm, 7 * bn), (64 * bm, 8 * bn), 512             # 511 / 512 tiles
        for tag, (M, N), tiles in (("below", lo, thr - 1), ("at", hi, thr)):
            for bounded in (False, True):
                body = f"p[0] = mk(0, {M}, {N}, 36, {fwd}); n = 1;" + (" p[0].m_dev = ibuf;" if bounded else "")
                on = tiles >= thr
                if row == "tiles":                                 # (the fp32 kernel takes the order over the real rows itself)
                    exp = _ok(1, tiles, [0, tiles], [N // bn], [M // bm], 0, 1, [3 | (32 if on else 0)])
                else:
                    exp = _ok(1, tiles, [0, tiles], [N // bn], [M // bm],
                              1 if (on and not bounded and row != "x2n") else 0, 1, [3])
                add(f"order_rows_{tag}{'_bounded' if bounded else ''}", row, body, exp)
        # ---- ... and the slab rule of weight-gradient launches (15 / 16 tiles; fp32: 63 / 64)
        if mm_ok:
            if row == "tiles":
                shapes = (("below", 192, 192, 7, 63), ("at", 256, 256, 4, 64))
            else:
                shapes = (("below", 300, 100, 5, 15), ("at", 129, 100, 8, 16))
            for tag, M, N, ns, tiles in shapes:
                for x2 in ((False, True) if row != "tiles" else (False,)):
                    f = (R & ~BF3B) | SPLITK | (X2 if x2 else 0)
                    body = f"p[0] = mk(2, {M}, {N}, 8192, {f}); p[0].nsplit = {ns}; n = 1;"
                    on = tag == "at"
                    if row == "tiles":
                        exp = _ok(1, tiles, [0, tiles], [cd(N, 64)], [cd(M, 64)], 0, 1, [SPLITK | (2048 if on else 0)])
                    else:
                        slab = on and (row == "b3p" or x2)
                        exp = _ok(1, tiles, [0, tiles], [1], [cd(M, 128)], 1 if slab else 0, 3, [SPLITK])
                    add(f"order_slabs_{tag}{'_x2' if x2 else ''}", row, body, exp)
        # ---- epilogue classes
        one = lambda lay, f: f"p[0] = mk({lay}, 300, 200, 36, {f}); n = 1;"
        g = [cd(200, bn)], [cd(300, bm)]
        t1 = g[0][0] * g[1][0]
        if row == "tiles":
            for tag, lay, f, e in (("fwd", 0, BIAS | SELU, 1), ("fwd_dselu", 0, DSELU, 0), ("dgrad", 1, DSELU, 1),
                                   ("dgrad_accum", 1, DSELU | ACCUM, 0), ("wgrad", 2, 0, 1), ("fwd_plain", 0, 0, 0)):
                add(f"epi_{tag}", row, one(lay, f), _ok(1, t1, [0, t1], *g, 0, e, [f]))
            add("epi_mixed", row, three + f" p[2].flags = {DSELU};", _ok(2, 35, [0, 20, 35], [4, 5], [5, 3], 0, 0, [3, DSELU]))
        else:
            plain = 3 if row in ("b3v", "b3p") else 0          # (bf3 / x2n compile classes 0-2)
            for tag, f, e in (("fwd", BIAS | SELU, 1), ("dgrad", DSELU, 2), ("plain", 0, plain), ("accum", ACCUM, 0),
                              ("mulact", BIAS | SELU | MULACT, 0)):
                add(f"epi_{tag}", row, one(0, R | f), _ok(1, t1, [0, t1], *g, 0, e, [f]))
            add("epi_mixed", row, three + f" p[2].flags = {R | DSELU};",
                _ok(2, t0 + t2, [0, t0, t0 + t2], [cd(200, bn), cd(257, bn)], [cd(300, bm), cd(130, bm)], 0, 0, [3, DSELU]))
            if mm_ok:
                add("epi_slabs_accum", row, odd + f" p[0].lda = 130; p[0].flags |= {ACCUM};",
                    _ok(1, mm_tiles, [0, mm_tiles], [cd(200, bn)], [cd(129, bm)], 0, 0, [SPLITK | ACCUM]))
                # fp16x2 slabs take a flag-free epilogue only on b3v
                add("x2_slabs_accum", row, odd + f" p[0].lda = 130; p[0].flags |= {ACCUM | X2};", EINVAL if row == "b3v" else
                    _ok(1, mm_tiles, [0, mm_tiles], [cd(200, bn)], [cd(129, bm)], 0, 0, [SPLITK | ACCUM]))
        # ---- nothing to launch; more tiles than a grid takes (0x3fffffff)
        add("empty", row, f"p[0] = mk(0, 0, 200, 36, {fwd}); n = 1;", "0 0 0 0 0 1")
        if mm_ok:
            add("tile_limit", row, odd + " p[0].lda = 130; p[0].nsplit = 1 << 30;", ELIMIT)
        else:       # (the 16-deep kernel's launcher used to add these up unchecked)
            add("tile_limit", row, f"p[0] = mk(0, 1 << 28, 1 << 26, 4, {fwd}); n = 1;", ELIMIT)
    return cases


def test_launch_plans_match_the_launchers_they_replace(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    cases = _cases()
    assert {row for _, row, _, _ in cases} == set(ROWS)
    src = [PROLOGUE, _caps_source(), "int main() {", "  gi_gemm_params p[8]; int n;"]
    for name, row, body, _ in cases:
        src.append(f"  {{ memset(p, 0, sizeof(p)); n = 0; {body} run(\"{name}\", {ROWS[row][1]}, p, n); }}")
    src += ["  return 0;", "}"]
    cfile, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    cfile.write_text("\n".join(src))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(cfile), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (no sanitizer runtime to link against: plain build)
        subprocess.run(base, check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    got = dict(line.split(" ", 1) for line in res.stdout.strip().split("\n"))
    assert len(got) == len(cases)
    wrong = [(name, got[name], exp) for name, _, _, exp in cases if got[name] != exp]
    assert not wrong, "\n".join(f"{n}: got [{g}] expected [{e}]" for n, g, e in wrong)
