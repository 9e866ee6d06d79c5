"""The kernels that the conv trunk's backward pass gained with the gather-form data gradients stay in registers and leave
room for a second block on the CU.

conv3's / conv2's data gradients are gemm_lds instantiations whose A loader decodes (frame, y, x, tap) per 16-byte load
(csrc/learner_common.h: ProbDgrad3, ProbDgrad2), and conv1's weight gradient of the f32x3 mode is gemm_bf16x3 with a
one-part B operand (gemm_bf16x3.h: SinglePartB).  All three hide their global-load latency only with a second block of 8
waves on the same CU, and index arithmetic that spills would put scratch traffic inside the chunk loop without any test of
the results noticing.  So the compiler's own account is asserted here (no GPU needed): csrc/learner.hip is compiled
device-only with build.py's HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage and for each of the three kernels the
remarks must say `ScratchSize [bytes/lane]: 0`, `VGPRs Spill: 0`, an occupancy of at least 4 waves per SIMD (a block is
2 waves per SIMD) and at most 80 KB of static LDS per block (two blocks in a CU's 160 KB).  Only the remarks are read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# substrings of the mangled kernel names: gemm_lds<.., ProbDgrad3>, gemm_lds<.., ProbDgrad2>, gemm_bf16x3<SinglePartB<..>, ProbW1>
KERNELS = {"dgrad_conv3": ("8gemm_ldsI", "10ProbDgrad3E"), "dgrad_conv2": ("8gemm_ldsI", "10ProbDgrad2E"),
           "wgrad_conv1_single_part_b": ("11gemm_bf16x3I", "11SinglePartBI", "6ProbW1E")}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of csrc/learner.hip's kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    obj = str(tmp_path_factory.mktemp("tbres") / "learner_dev.o")
    cmd = [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                   os.path.join(b.CSRC, "learner.hip"), "-o", obj]
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


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_two_blocks_per_cu(resources, kernel):
    mine = {n: v for n, v in resources.items() if all(part in n for part in KERNELS[kernel])}
    assert len(mine) == 1, (kernel, sorted(resources))
    (name, v), = mine.items()
    print(name, v)
    assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
    assert v["VGPRs Spill"] == 0, (name, v)
    assert v["Occupancy [waves/SIMD]"] >= 4, (name, v)  # (8 waves per block over 4 SIMDs: two blocks need four)
    assert v["LDS Size [bytes/block]"] <= 80 * 1024, (name, v)
