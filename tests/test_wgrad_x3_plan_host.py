"""The wgrad_x3 option where there is no GPU: the learners' backward plan (rela_amd/csrc/learner_plan.h; the members it must
not move are pinned to the parent's tables by tests/test_learner_plan_host.py), the block-count functions, the compiler's
account of the two kernels, and --learner_wgrad of the training entry points."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "wgrad_x3_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "libwgrad_x3_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "learner_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


@pytest.mark.parametrize("learner,precision,two_lanes",
                         [(0, p, lanes) for p in (0, 1, 2) for lanes in (0, 1)] + [(1, p, 0) for p in (0, 1, 2, 3)])
def test_the_option_sets_its_members_and_nothing_else(shim, learner, precision, two_lanes):
    for frames in (1, 512, 1024, 1025, 2047, 2048, 5312):
        for dgrad_x3 in (0, 1):
            off, on = (C.c_int * 15)(), (C.c_int * 15)()
            shim.shim_trunk_plan_wx3(learner, precision, two_lanes, frames, dgrad_x3, 0, off)
            shim.shim_trunk_plan_wx3(learner, precision, two_lanes, frames, dgrad_x3, 1, on)
            assert list(on)[:12] == list(off)[:12] and off[11] == dgrad_x3, (frames, list(off), list(on))
            assert list(off)[12:] == [0, 0, 0], (frames, list(off))
            assert list(on)[12:] == [1, shim.shim_wgrad1_x3_blocks(frames, two_lanes), shim.shim_wgrad2_x3_blocks(frames)]


def test_block_counts_at_their_break_points(shim):
    """a frame per block up to 256 blocks; conv1 on two lanes up to 128"""
    for frames, one, two in ((1, 1, 1), (127, 127, 127), (128, 128, 128), (129, 129, 128), (255, 255, 128), (256, 256, 128),
                             (257, 256, 128), (5312, 256, 128)):
        assert (shim.shim_wgrad1_x3_blocks(frames, 0), shim.shim_wgrad1_x3_blocks(frames, 1)) == (one, two), frames
        assert shim.shim_wgrad2_x3_blocks(frames) == one, frames


def test_the_two_kernels_have_no_scratch(tmp_path):
    """csrc/wgrad_conv_x3.hip with the build's flags: both kernels at two waves per SIMD, as the header says"""
    from kernel_resources import kernel_resources

    res = kernel_resources("wgrad_conv_x3.hip", tmp_path)
    for kernel in ("wgrad_conv1_x3", "wgrad_conv2_x3"):
        (v,) = [v for n, v in res.items() if kernel in n]
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (kernel, v)
        assert v["Occupancy [waves/SIMD]"] >= 2, (kernel, v)


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_learner_wgrad_flag_and_its_refusal(algo):
    from rela_amd.pyrela import main as entry

    assert entry.learner_wgrad_x3(entry.parse_args(["--algo", algo, "--hip_learner", "0"])) is False  # default: mode
    assert entry.learner_wgrad_x3(entry.parse_args(["--algo", algo, "--learner_wgrad", "x3"])) is True
    with pytest.raises(SystemExit):
        entry.parse_args(["--learner_wgrad", "x2"])
    with pytest.raises(SystemExit) as e:
        entry.train(entry.parse_args(["--algo", algo, "--hip_learner", "0", "--learner_wgrad", "x3"]))
    assert "--learner_wgrad x3" in str(e.value) and "--hip_learner 1" in str(e.value)
