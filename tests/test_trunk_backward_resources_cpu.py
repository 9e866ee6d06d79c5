"""The kernels that the conv trunk's backward pass gained with the gather-form data gradients stay in registers and leave
room for a second block on the CU.

conv3's / conv2's data gradients are gemm_lds instantiations whose A loader decodes (frame, y, x, tap) per 16-byte load
(csrc/learner_common.hip: ProbDgrad3, ProbDgrad2), and conv1's weight gradient of the f32x3 mode is gemm_bf16x3 with a
one-part B operand (gemm_bf16x3.h: SinglePartB).  All three hide their global-load latency only with a second block of 8
waves on the same CU, and index arithmetic that spills would put scratch traffic inside the chunk loop without any test of
the results noticing.  So the compiler's own account is asserted here (no GPU needed): csrc/learner_common.hip, the one
unit that holds the trunk's backward pass for both learners, is compiled device-only with build.py's HIP_FLAGS plus
-Rpass-analysis=kernel-resource-usage and for each of the three kernels the remarks must say `ScratchSize [bytes/lane]: 0`, `VGPRs Spill: 0`, an occupancy of at least 4 waves per SIMD (a block is
2 waves per SIMD) and at most 80 KB of static LDS per block (two blocks in a CU's 160 KB).  Only the remarks are read.
"""
import pytest

from kernel_resources import kernel_resources

# substrings of the mangled kernel names: gemm_lds<.., ProbDgrad3>, gemm_lds<.., ProbDgrad2>, gemm_bf16x3<SinglePartB<..>, ProbW1>
KERNELS = {"dgrad_conv3": ("8gemm_ldsI", "10ProbDgrad3E"), "dgrad_conv2": ("8gemm_ldsI", "10ProbDgrad2E"),
           "wgrad_conv1_single_part_b": ("11gemm_bf16x3I", "11SinglePartBI", "6ProbW1E")}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of csrc/learner_common.hip's kernels"""
    return kernel_resources("learner_common.hip", tmp_path_factory.mktemp("tbres"))


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
