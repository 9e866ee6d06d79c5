"""The wgrad3_x3 option where there is no GPU: the learners' backward plan (rela_amd/csrc/learner_plan.h), the block-count
function and the compiler's account of the kernel."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "wgrad3_x3_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "libwgrad3_x3_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "learner_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


def test_block_count_at_its_break_points(shim):
    """a frame per block up to 256 blocks"""
    for frames, blocks in ((1, 1), (255, 255), (256, 256), (257, 256), (32768, 256)):
        assert shim.shim_wgrad3_x3_blocks(frames) == blocks, frames


@pytest.mark.parametrize("learner,precision,two_lanes",
                         [(0, p, lanes) for p in (0, 1, 2) for lanes in (0, 1)] + [(1, p, 0) for p in (0, 1, 2, 3)])
def test_the_option_sets_its_members_and_nothing_else(shim, learner, precision, two_lanes):
    """off: the plan of the calls without the new parameter, for every combination of the other three options; on: the same
    plan but for the two new members"""
    for frames in (1, 512, 1024, 1025, 2047, 2048, 5312):
        for others in (0, 1, 2, 3, 8, 9, 10, 11) if learner else (0, 1, 2, 3):  # (bits 0, 1 and, for R2D2, 3)
            before, off, on = (C.c_int * 17)(), (C.c_int * 17)(), (C.c_int * 17)()
            shim.shim_trunk_plan_before(learner, precision, two_lanes, frames, others, before)
            shim.shim_trunk_plan_w3x3(learner, precision, two_lanes, frames, others, off)
            shim.shim_trunk_plan_w3x3(learner, precision, two_lanes, frames, others | 4, on)
            assert list(off) == list(before) and list(off)[15:] == [0, 0], (frames, others, list(before), list(off))
            assert list(on)[:15] == list(off)[:15] and list(on)[15:] == [1, shim.shim_wgrad3_x3_blocks(frames)], (frames, list(on))


def test_the_kernel_has_no_scratch(tmp_path):
    """csrc/wgrad_conv3_x3.hip with the build's flags: two waves per SIMD, as the header says.  (The kernel's LDS is dynamic:
    the remark counts static LDS, and the header's static_assert holds the 142,848 B it asks for at the launch.)"""
    from kernel_resources import kernel_resources

    ((v,),) = [[v for n, v in kernel_resources("wgrad_conv3_x3.hip", tmp_path).items() if "wgrad_conv3_x3" in n]]
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["Occupancy [waves/SIMD]"] >= 2 and v["LDS Size [bytes/block]"] <= 163840, v
