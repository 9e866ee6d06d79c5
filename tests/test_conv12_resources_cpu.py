"""conv12_s3 (csrc/conv12_s3.h) keeps everything in registers: no scratch, no spills, in either instantiation.

The kernel holds 240 weight registers per wave with one wave per SIMD.  conv2's 192 are pinned into the accumulator half
of the register file (they are MFMA A operands only), so that the frame loop's addresses, staging registers and
fragment rings have the 256 architectural VGPRs to themselves.  One more hoisted offset or a deeper ring can tip the
allocator back into spilling the loop's values -- scratch traffic inside conv1's MFMA phase -- without any test of the
results noticing, so the compiler's own account is asserted here (no GPU needed):

csrc/ffnet.hip is compiled device-only with build.py's HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage (about half
a minute) and, for conv12_s3<false> (the actors' and the target net's forward) and conv12_s3<true> (the learner's
online(obs) pass, which also writes a1 as f32), the remarks must say `ScratchSize [bytes/lane]: 0` and `VGPRs Spill: 0`.
Only the remarks are read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONV12 = ("conv12_s3ILb0E", "conv12_s3ILb1E")  # <false>, <true> in the mangled names


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of csrc/ffnet.hip's kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    obj = str(tmp_path_factory.mktemp("c12res") / "ffnet_dev.o")
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


@pytest.mark.parametrize("inst", CONV12)
def test_conv12_s3_no_scratch_no_spills(resources, inst):
    mine = {n: v for n, v in resources.items() if inst in n}  # (the mangled kernel name with its template argument)
    assert len(mine) == 1, sorted(resources)
    (name, v), = mine.items()
    print(name, v)
    assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
    assert v["VGPRs Spill"] == 0, (name, v)
    assert v["Occupancy [waves/SIMD]"] == 1, (name, v)  # (512 registers per lane: one wave per SIMD, four per CU)
