"""The dgrad_x3 option where there is no GPU: the learners' backward plan (rela_amd/csrc/learner_plan.h; the members it must
not move are pinned to the parent's tables by tests/test_learner_plan_host.py), the compiler's account of the two kernels,
and --learner_dgrad of the training entry points."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "dgrad_x3_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "libdgrad_x3_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "learner_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


@pytest.mark.parametrize("learner,precision,two_lanes",
                         [(0, p, lanes) for p in (0, 1, 2) for lanes in (0, 1)] + [(1, p, 0) for p in (0, 1, 2, 3)])
def test_the_option_sets_its_member_and_nothing_else(shim, learner, precision, two_lanes):
    for frames in (1, 512, 1024, 1025, 2047, 2048, 5312):
        off, on = (C.c_int * 12)(), (C.c_int * 12)()
        shim.shim_trunk_plan_x3(learner, precision, two_lanes, frames, 0, off)
        shim.shim_trunk_plan_x3(learner, precision, two_lanes, frames, 1, on)
        assert off[11] == 0 and on[11] == 1 and list(on)[:11] == list(off)[:11], (frames, list(off), list(on))
        assert off[10] == int(precision == 1)  # dgrad_bf16 keeps its meaning and value


def test_the_two_kernels_have_no_scratch(tmp_path):
    """csrc/dgrad_conv_x3.hip with the build's flags for that file: conv2 at two waves per SIMD, conv3 at one"""
    from kernel_resources import device_only_cmd, parse_remarks
    from rela_amd import build as b

    cmd = device_only_cmd("dgrad_conv_x3.hip", str(tmp_path / "dgrad_conv_x3_dev.o"))
    cmd[1:1] = b.EXTRA_HIP_FLAGS["dgrad_conv_x3.hip"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res = parse_remarks(r.stderr)
    for kernel, waves in (("dgrad_conv2_x3", 2), ("dgrad_conv3_x3", 1)):
        (v,) = [v for n, v in res.items() if kernel in n]
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (kernel, v)
        assert v["Occupancy [waves/SIMD]"] >= waves, (kernel, v)


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_learner_dgrad_flag_and_its_refusal(algo):
    from rela_amd.pyrela import main as entry

    assert entry.learner_dgrad_x3(entry.parse_args(["--algo", algo, "--hip_learner", "0"])) is False  # default: mode
    assert entry.learner_dgrad_x3(entry.parse_args(["--algo", algo, "--learner_dgrad", "x3"])) is True
    with pytest.raises(SystemExit):
        entry.parse_args(["--learner_dgrad", "x2"])
    with pytest.raises(SystemExit) as e:
        entry.train(entry.parse_args(["--algo", algo, "--hip_learner", "0", "--learner_dgrad", "x3"]))
    assert "--learner_dgrad x3" in str(e.value) and "--hip_learner 1" in str(e.value)
    with pytest.raises(SystemExit) as e:  # f32x3_bwd stays the R2D2 learner's mode, with or without the option
        entry.train(entry.parse_args(["--algo", "apex", "--learner_precision", "f32x3_bwd", "--learner_dgrad", "x3"]))
    assert "--algo r2d2" in str(e.value)
