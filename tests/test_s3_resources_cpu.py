"""Register budget of the f32x3 kernels, read from the compiler (no GPU needed).

csrc/ffnet.hip is compiled device-only with build.py's HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage (about half
a minute) and the remarks are checked:

  * every instantiation of s3::gemm_s3 (csrc/gemm_s3.h) runs two waves per SIMD with no scratch: `ScratchSize 0`,
    `VGPRs Spill 0`, `Occupancy [waves/SIMD] 2`.  The kernel's schedule (eight waves per block, a partner wave issuing
    MFMAs while the other issues its loads) rests on that: one more accumulator tile or a deeper fragment ring would
    silently drop it back to one wave per SIMD or to spills;
  * conv12_s3 / conv3_img_s3 do not get worse than they are: a ceiling of 40 B (conv12_s3<false>), 152 B (conv12_s3<true>)
    and 0 B (conv3_img_s3) of scratch per lane, so that a later change cannot add spills unnoticed.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scratch ceilings [bytes/lane] of the convolution kernels (what they had when gemm_s3 went to eight waves)
CONV_SCRATCH_CEILING = {"conv12_s3ILb0E": 40, "conv12_s3ILb1E": 152, "conv3_img_s3": 0}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of csrc/ffnet.hip's kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    obj = str(tmp_path_factory.mktemp("s3res") / "ffnet_dev.o")
    cmd = [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                   os.path.join(b.CSRC, "ffnet.hip"), "-o", obj]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_gemm_s3_two_waves_per_simd_no_scratch(resources):
    gemms = {n: v for n, v in resources.items() if "s37gemm_s3I" in n}
    # fc (ReLU; raw sums for split-K) and the gate GEMM (raw sums; bias): the four instantiations ffnet.hip launches
    assert len(gemms) >= 4, sorted(resources)
    for name, v in gemms.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] == 2, (name, v)


def test_conv_s3_scratch_does_not_grow(resources):
    seen = set()
    for name, v in resources.items():
        for key, ceiling in CONV_SCRATCH_CEILING.items():
            if "2s3" in name and key in name:
                seen.add(key)
                print(name, v)
                assert v["ScratchSize [bytes/lane]"] <= ceiling, (name, v)
    assert seen == set(CONV_SCRATCH_CEILING), sorted(resources)
