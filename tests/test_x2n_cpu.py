"""CPU (no GPU needed): the fp16x2 kernels the model launches compile without VGPR spills and without scratch —
hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on the sources, with the library's own flags.
Covered: every instantiation of the forward / dgrad kernel (csrc/gi_gemm_x2n.hip), the fp16x2 instantiations of
gi_gemm_bf3_kernel (template argument X2 = true) and of gi_b3p_kernel (X2 = true: the weight gradients)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphinvent_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (source, extra flags as in csrc/Makefile, pattern of the mangled kernel names to check)
CASES = [
    ("gi_gemm_x2n.hip", [], r"gi_gemm_x2n_kernel"),
    ("gi_gemm_bf3.hip", [], r"gi_gemm_bf3_kernelILi\dELb\dELb\dELb1EE"),
    ("gi_gemm_b3p.hip", ["-fno-slp-vectorize"], r"gi_b3p_kernelILb\dELb\dELi\dELb1E"),
]


def _usage(src, extra, tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Wall", "-Wno-unused-function", *extra, "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, src), "-o", str(tmp_path / "k.o")]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|AGPRs): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    return kernels


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src,extra,pattern", CASES, ids=[c[0] for c in CASES])
def test_fp16x2_kernels_do_not_spill(src, extra, pattern, tmp_path):
    kernels = _usage(src, extra, tmp_path)
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert hit, f"no kernel of {src} matches {pattern}: {sorted(kernels)}"
    for k, v in hit.items():
        assert v.get("VGPRs Spill") == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]") == 0, (k, v)
    if src == "gi_gemm_x2n.hip":          # the occupancy the kernel declares: three workgroups of 4 waves per CU
        assert len(hit) == 2
        for k, v in hit.items():
            assert v["VGPRs"] + v.get("AGPRs", 0) <= 168, (k, v)
