"""CPU: the resources the compiler gives the four job kernels, read from the code object metadata of the device pass (no GPU needed:
hipcc cross-compiles for gfx950).  The single-wave kernel k_job is compiled for five waves per SIMD, which needs at most 96 VGPRs, and
20 of its workgroups must fit a CU's LDS; the multi-wave kernels keep 128 VGPRs.  The bounds are the ones of profiles/r18/README.md.
Numbers only: nothing here looks at instructions."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "linear_amd", "csrc", "lnr_api.hip")

K_JOB_VGPRS = 96            # five waves per SIMD: 512 / 5 rounded down to the granule of 8
K_JOB_STATIC_LDS = 2616     # LeaderScratch (2304) + the DP tile's leaf flags (272) + 40 B of counters: with the 4 KB arena 6712 B, 20 workgroups need 8192 or less each
K_JOB_PRIVATE = 696         # bytes of private segment per lane (the parent had 1088 at 128 VGPRs)
MULTI_WAVE = ("k_job_heavy", "k_job_mid", "k_job_mid2")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    from linear_amd import build as lb
    try:
        hipcc = lb.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("job_resources") / "api.s")
    flags = [f for f in lb.FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", API, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count.*?\.wavefront_size:\s+\d+", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN3lnr\d+(k_job\w*?)ENS_7JobArgsE$", name)
        if m:
            res[m.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    print(res)
    assert set(res) == {"k_job"} | set(MULTI_WAVE), sorted(res)
    return res


def test_k_job_fits_five_waves_per_simd(kernels):
    assert kernels["k_job"]["vgpr_count"] <= K_JOB_VGPRS, kernels["k_job"]


def test_k_job_static_lds(kernels):
    assert kernels["k_job"]["group_segment_fixed_size"] <= K_JOB_STATIC_LDS, kernels["k_job"]


def test_k_job_private_segment(kernels):
    assert kernels["k_job"]["private_segment_fixed_size"] <= K_JOB_PRIVATE, kernels["k_job"]


@pytest.mark.parametrize("name", MULTI_WAVE)
def test_multi_wave_kernels_keep_128_vgprs(kernels, name):
    assert kernels[name]["vgpr_count"] == 128, kernels[name]
