"""CPU checks of the R2D2 learner's "f32x3_bwd" mode (tests/test_r2d2_learner_bwd_mode_gpu.py has the GPU half).

Resources: mode 3 instantiates gemm_bf16x3 (csrc/gemm_bf16x3.h) with three-part 64 x 64 tiles for three Problems of
csrc/learner_r2d2.hip -- ProbWhh, ProbWih, ProbIhDgrad -- next to the conv weight gradients' three, which both learners
run from csrc/learner_common.hip.  A block holds four
register sets of staged loads next to two accumulators per 16 x 16 tile and runs with a second block on its CU; a spill would
put scratch traffic inside the chunk loop without any test of the results noticing.  So the compiler's own account is asserted
(as tests/test_trunk_backward_resources_cpu.py does for csrc/learner_common.hip): both files are compiled device-only
with build.py's HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage, and every three-part gemm_bf16x3 kernel of
learner_r2d2.hip and the three conv weight gradients of learner_common.hip must report `ScratchSize [bytes/lane]: 0`, `VGPRs Spill: 0`, `SGPRs Spill: 0` and an occupancy of at least 4 waves per
SIMD (a block is 2: the tiles were chosen for two blocks per CU).  Only the remarks are read.

Arguments: rela_amd/pyrela/main.py's --learner_precision and its two refusals.
"""
import re

import pytest

from kernel_resources import kernel_resources

# mangled: gemm_bf16x3<TileCfg<BM, BN, WM, WN, AMC, 3, S>, Problem>
THREE_PART = re.compile(r"11gemm_bf16x3I.*7TileCfgILi\d+ELi\d+ELi\d+ELi\d+ELb[01]ELi3ELi\d+EE")
NEW_PROBLEMS = ("7ProbWhhE", "7ProbWihE", "11ProbIhDgradE")


# the conv weight gradients (conv3, conv2: ProbConvWgrad; conv1: ProbW1), compiled in csrc/learner_common.hip
CONV_WGRADS = ("13ProbConvWgradI", "6ProbW1E")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of the three-part gemm_bf16x3 kernels an R2D2 step can launch: all of
    csrc/learner_r2d2.hip's, and the conv weight gradients' of csrc/learner_common.hip"""
    tmp = tmp_path_factory.mktemp("r2d2res")
    own = {n: v for n, v in kernel_resources("learner_r2d2.hip", tmp).items() if THREE_PART.search(n)}
    trunk = {n: v for n, v in kernel_resources("learner_common.hip", tmp).items()
             if THREE_PART.search(n) and any(p in n for p in CONV_WGRADS)}
    assert own and not set(own) & set(trunk)
    return {**own, **trunk}


def test_three_part_gemms_have_no_scratch_and_no_spills(resources):
    mine = resources
    for prob in NEW_PROBLEMS:
        assert sum(prob in n for n in mine) == 1, (prob, sorted(mine))
    assert sum(any(p in n for p in CONV_WGRADS) for n in mine) == 3, sorted(mine)  # conv3, conv2, conv1
    for name, v in sorted(mine.items()):
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (name, v)  # (8 waves per block over 4 SIMDs: two blocks need four)


@pytest.fixture(scope="module")
def entry():
    from rela_amd.pyrela import main

    return main


def test_learner_precision_flag_parses_and_defaults_to_f32(entry):
    assert entry.parse_args([]).learner_precision == "f32"
    for mode in ("f32", "bf16x2", "f32x3", "f32x3_bwd"):
        args = entry.parse_args(["--algo", "r2d2", "--learner_precision", mode])
        assert args.learner_precision == mode and entry.learner_precision(args) == mode
    for mode in ("f32", "bf16x2", "f32x3"):
        assert entry.learner_precision(entry.parse_args(["--algo", "apex", "--learner_precision", mode])) == mode
    with pytest.raises(SystemExit):
        entry.parse_args(["--learner_precision", "fp8"])


@pytest.mark.parametrize("argv", [["--algo", "apex", "--learner_precision", "f32x3_bwd"],
                                  ["--algo", "r2d2", "--hip_learner", "0", "--learner_precision", "f32x3_bwd"],
                                  ["--algo", "r2d2", "--hip_learner", "0", "--learner_precision", "f32x3"],
                                  ["--algo", "apex", "--hip_learner", "0", "--learner_precision", "bf16x2"]],
                         ids=lambda a: " ".join(a))
def test_learner_precision_refusals(entry, argv, capsys):
    """f32x3_bwd with --algo apex, and anything but f32 with --hip_learner 0: train() and train_multi() end with a
    SystemExit that says why, before anything is built; f32 with --hip_learner 0 passes the check."""
    args = entry.parse_args(argv)
    for run in (entry.train, entry.train_multi):
        with pytest.raises(SystemExit) as e:
            run(args)
        assert "--learner_precision" in str(e.value) and ("--hip_learner 1" in str(e.value) or "--algo r2d2" in str(e.value))
    assert entry.learner_precision(entry.parse_args(["--hip_learner", "0"])) == "f32"
