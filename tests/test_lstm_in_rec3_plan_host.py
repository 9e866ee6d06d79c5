"""The lstm_in_rec3 option where there is no GPU: the R2D2 learner's backward plan (rela_amd/csrc/learner_plan.h), the
compiler's account of gemm_rec3_nt (csrc/gemm_rec3.hip) and --learner_lstm_in of the training entry point."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# the plan before the option: heads, head_wgrad_splits (below, from 1024 rows), lstm_in_rec64, lstm_in, trunk: arith, muls, lanes
PARENT_PLAN = {0: (0, (1, 32), 0, 0, 0, 1, 1, 1, 0), 1: (0, (1, 32), 1, 0, 1, 1, 1, 1, 0), 2: (0, (1, 32), 0, 0, 0, 1, 1, 1, 0),
               3: (0, (1, 32), 0, 2, 2, 2, 2, 2, 0)}


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "lstm_in_rec3_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "liblstm_in_rec3_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "learner_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


@pytest.mark.parametrize("precision", [0, 1, 2, 3])
def test_the_option_sets_its_member_and_nothing_else(shim, precision):
    def plan(*args):
        out = (C.c_int * 11)()
        shim.shim_r2d2_plan_rec3(precision, *args, out)
        return list(out)

    for rows in (1, 1023, 1024, 1025, 5312):
        for dgrad_x3 in (0, 1):
            before, off, on = plan(rows, dgrad_x3, 0, 0), plan(rows, dgrad_x3, 1, 0), plan(rows, dgrad_x3, 1, 1)
            want = [v[rows >= 1024] if isinstance(v, tuple) else v for v in PARENT_PLAN[precision]]
            assert before == want + [dgrad_x3, 0], (rows, before)
            assert off == before and on == before[:10] + [1], (rows, off, on)


def test_the_kernels_have_no_scratch_and_two_waves_per_simd(tmp_path):
    """csrc/gemm_rec3.hip with the build's flags: row tile 256 / 128 x EpiPlain / EpiReluMask, no scratch, two waves per SIMD"""
    from kernel_resources import kernel_resources

    res = {n: v for n, v in kernel_resources("gemm_rec3.hip", tmp_path).items() if "gemm_rec3_nt" in n}
    assert len(res) == 4 and sum("ILi256E" in n for n in res) == 2 and sum("EpiReluMask" in n for n in res) == 2, sorted(res)
    for name, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (name, v)


def test_learner_lstm_in_flag_and_its_refusals():
    from rela_amd.pyrela import main as entry

    assert entry.learner_lstm_in_rec3(entry.parse_args(["--algo", "r2d2"])) is False  # default: mode
    assert entry.learner_lstm_in_rec3(entry.parse_args(["--algo", "r2d2", "--learner_lstm_in", "rec3"])) is True
    with pytest.raises(SystemExit):
        entry.parse_args(["--learner_lstm_in", "rec2"])
    for argv, needs in ((["--algo", "r2d2", "--hip_learner", "0"], "--hip_learner 1"), (["--algo", "apex"], "--algo r2d2")):
        with pytest.raises(SystemExit) as e:
            entry.train(entry.parse_args(argv + ["--learner_lstm_in", "rec3"]))
        assert needs in str(e.value)
