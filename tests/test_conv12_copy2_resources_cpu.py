"""conv12_s3_copy2 (csrc/conv12_s3.h; the symbol is conv12_s3_copies2) fits the register file like conv12_s3_copy.

conv12_s3_copy2 is conv12_s3_copy plus eight 16-byte global loads and eight stores per thread and frame, which pass a
second frame through four rotating registers under the MFMAs.  conv12_s3 holds 240 weight registers per wave with one
wave per SIMD, and a few more live values across the frame loop have tipped its allocation into scratch before
(tests/test_conv12_resources_cpu.py), so the compiler's own account is asserted, from the resource remarks of a
device-only compile of csrc/ffnet.hip for gfx950 (no GPU needed; only the remarks are read):

  * no scratch, no spilled registers, occupancy 1 (one block of four waves per CU), 256 accumulator registers;
  * the static LDS of conv12_s3_copy (none: the 160,352 bytes are dynamic, and the launcher passes the same figure);
  * at most 16 VGPRs over conv12_s3_copy: the four rotating registers, not a second staged frame (32).

What the existing instantiations report is held by tests/test_conv12_copy_resources_cpu.py.
"""
import pytest

from kernel_resources import kernel_resources

COPY2, COPY = "conv12_s3_copies2", "conv12_s3_copyE"


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    return kernel_resources("ffnet.hip", tmp_path_factory.mktemp("c12copy2"))


def _one(resources, key):
    mine = {n: v for n, v in resources.items() if key in n}
    assert len(mine) == 1, sorted(resources)
    (name, v), = mine.items()
    print(name, v)
    return name, v


def test_copy2_no_scratch_no_spills_one_block_per_cu(resources):
    name, v = _one(resources, COPY2)
    assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    assert v["Occupancy [waves/SIMD]"] == 1, (name, v)
    assert v["AGPRs"] == 256, (name, v)


def test_copy2_lds_and_registers_against_the_copy_variant(resources):
    name, v = _one(resources, COPY2)
    _, c = _one(resources, COPY)
    assert v["LDS Size [bytes/block]"] == c["LDS Size [bytes/block]"], (name, v, c)
    assert v["VGPRs"] <= c["VGPRs"] + 16, (name, v, c)
