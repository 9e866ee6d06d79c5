"""conv12_s3_copy (csrc/conv12_s3.h) fits the register file like the kernel it extends, and leaves that kernel alone.

conv12_s3_copy is conv12_s3<false> plus eight 16-byte global stores per thread and frame from the registers the staged
frame already sits in.  conv12_s3 holds 240 weight registers per wave with one wave per SIMD, and one more live value
across the frame loop has tipped its allocation into scratch before (tests/test_conv12_resources_cpu.py), so the
compiler's own account is asserted, from the resource remarks of a device-only compile of csrc/ffnet.hip for gfx950 (no
GPU needed; only the remarks are read):

  * conv12_s3_copy: no scratch, no spilled registers, occupancy 1 (one block of four waves per CU), 256 accumulator
    registers (conv2's pinned weights) like the others;
  * conv12_s3<false> and conv12_s3<true> report the registers and LDS they reported before the copy variant existed
    (200 / 202 VGPRs, 256 AGPRs, no static LDS: the 160,352 bytes are dynamic).  Both are the same inlined body with the
    copy compiled out; these numbers moving would mean the shared body no longer compiles to the same kernel.
"""
import pytest

from kernel_resources import kernel_resources

COPY = "conv12_s3_copy"
PLAIN = {"conv12_s3ILb0E": {"VGPRs": 200, "AGPRs": 256, "LDS Size [bytes/block]": 0},   # <false>
         "conv12_s3ILb1E": {"VGPRs": 202, "AGPRs": 256, "LDS Size [bytes/block]": 0}}   # <true>


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    return kernel_resources("ffnet.hip", tmp_path_factory.mktemp("c12copy"))


def _one(resources, key):
    mine = {n: v for n, v in resources.items() if key in n}
    assert len(mine) == 1, sorted(resources)
    (name, v), = mine.items()
    print(name, v)
    return name, v


def test_copy_variant_no_scratch_no_spills_one_block_per_cu(resources):
    name, v = _one(resources, COPY)
    assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    assert v["Occupancy [waves/SIMD]"] == 1, (name, v)
    assert v["AGPRs"] == 256, (name, v)


@pytest.mark.parametrize("inst", sorted(PLAIN))
def test_existing_instantiations_keep_their_resources(resources, inst):
    name, v = _one(resources, inst)
    for key, want in PLAIN[inst].items():
        assert v[key] == want, (name, key, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] == 1, (name, v)
