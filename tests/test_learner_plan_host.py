"""Host-logic tests of the learners' backward plan (rela_amd/csrc/learner_plan.h): which kernel, which arithmetic and how
many split-K slices every weight gradient of the conv trunk runs with, and what the Ape-X and the R2D2 learner make of
their precision modes -- the pure functions rela_apex_learner_grad, rela_r2d2_learner_grad and the four backward taps call
before they launch anything.

tests/cpu_shims/learner_plan_host.cpp puts that header behind a C ABI.  The expected values are written out here as literals,
read off the launch code as it stood before the plan existed (csrc/learner_common.h trunk_backward, csrc/learner.hip
rela_apex_learner_grad, csrc/learner_r2d2.hip rela_r2d2_learner_grad at 8d3b014); nothing is computed from the header.
CPU-only.
"""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

F32, BF16X2, F32X3 = 0, 1, 2
FRAMES = [1, 512, 1024, 1025, 2047, 2048, 5312]
KERNEL = "bf16 kernel"  # wgrad_conv{1,2,3}_bf16.h; else (arithmetic of the GEMM, split-K slices)

# (arith, frames) -> (conv3, conv2, conv1) with multipliers 1, 1, 1 and fast_wgrad_min_frames = 2,048
TRUNK = {
    (F32, 1): ((F32, 84), (F32, 81), (F32, 64)),
    (F32, 512): ((F32, 84), (F32, 81), (F32, 64)),
    (F32, 1024): ((F32, 84), (F32, 81), (F32, 64)),
    (F32, 1025): ((F32, 28), (F32, 27), (F32, 64)),
    (F32, 2047): ((F32, 28), (F32, 27), (F32, 64)),
    (F32, 2048): ((F32, 28), (F32, 27), (F32, 64)),
    (F32, 5312): ((F32, 28), (F32, 27), (F32, 64)),
    (BF16X2, 1): ((BF16X2, 84), (BF16X2, 81), KERNEL),
    (BF16X2, 512): ((BF16X2, 84), (BF16X2, 81), KERNEL),
    (BF16X2, 1024): ((BF16X2, 84), (BF16X2, 81), KERNEL),
    (BF16X2, 1025): ((BF16X2, 28), (BF16X2, 27), KERNEL),
    (BF16X2, 2047): ((BF16X2, 28), (BF16X2, 27), KERNEL),
    (BF16X2, 2048): (KERNEL, KERNEL, KERNEL),
    (BF16X2, 5312): (KERNEL, KERNEL, KERNEL),
    (F32X3, 1): ((F32X3, 84), (F32X3, 81), (F32X3, 64)),
    (F32X3, 512): ((F32X3, 84), (F32X3, 81), (F32X3, 64)),
    (F32X3, 1024): ((F32X3, 84), (F32X3, 81), (F32X3, 64)),
    (F32X3, 1025): ((F32X3, 28), (F32X3, 27), (F32X3, 64)),
    (F32X3, 2047): ((F32X3, 28), (F32X3, 27), (F32X3, 64)),
    (F32X3, 2048): ((F32X3, 28), (F32X3, 27), (F32X3, 64)),
    (F32X3, 5312): ((F32X3, 28), (F32X3, 27), (F32X3, 64)),
}
# f32x3 with the R2D2 learner's mode-3 multipliers 2, 2, 2: conv1 doubled at every frame count, conv2 / conv3 above 1,024
# frames (below, their splits are tripled already)
TRUNK_X3_MUL2 = {
    1: ((F32X3, 84), (F32X3, 81), (F32X3, 128)),
    512: ((F32X3, 84), (F32X3, 81), (F32X3, 128)),
    1024: ((F32X3, 84), (F32X3, 81), (F32X3, 128)),
    1025: ((F32X3, 56), (F32X3, 54), (F32X3, 128)),
    2047: ((F32X3, 56), (F32X3, 54), (F32X3, 128)),
    2048: ((F32X3, 56), (F32X3, 54), (F32X3, 128)),
    5312: ((F32X3, 56), (F32X3, 54), (F32X3, 128)),
}
# ... and with (conv1, conv2, conv3) = (2, 3, 4): every multiplier reaches its own layer
TRUNK_X3_MUL234 = {1024: ((F32X3, 84), (F32X3, 81), (F32X3, 128)), 1025: ((F32X3, 112), (F32X3, 81), (F32X3, 128))}
W1_BLOCKS = {False: 256, True: 128}  # wgrad_conv1_bf16's block cap: w1fast::kMaxBlocks on one lane, 128 on two


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "learner_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "liblearner_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "learner_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


def _trunk(vals):
    """the 11 ints of the shim's put_trunk -> ((conv3, conv2, conv1) in the tables' form, conv1's block cap, dgrad on bf16)"""
    layers = tuple(KERNEL if vals[3 * i] else (vals[3 * i + 1], vals[3 * i + 2]) for i in range(3))
    return layers, vals[9], bool(vals[10])


def trunk_plan(shim, arith, frames, min_frames=2048, mul=(1, 1, 1), two_lanes=False):
    out = (C.c_int * 11)()
    shim.shim_plan_trunk_backward(arith, frames, min_frames, mul[0], mul[1], mul[2], int(two_lanes), out)
    return _trunk(list(out))


def apex_plan(shim, precision, two_lanes, frames):
    out = (C.c_int * 12)()
    shim.shim_plan_apex_backward(precision, int(two_lanes), frames, out)
    return out[0], _trunk(list(out)[1:])


def r2d2_plan(shim, precision, rows):
    out = (C.c_int * 15)()
    shim.shim_plan_r2d2_backward(precision, rows, out)
    v = list(out)
    return {"heads": v[0], "head_wgrad_splits": v[1], "rec64": bool(v[2]), "lstm_in": v[3]}, _trunk(v[4:])


def test_constants(shim):
    out = (C.c_int * 5)()
    shim.shim_constants(out)
    assert list(out) == [F32, BF16X2, F32X3, 8, 2048]


@pytest.mark.parametrize("two_lanes", [False, True], ids=["one-lane", "two-lanes"])
@pytest.mark.parametrize("arith", [F32, BF16X2, F32X3], ids=["f32", "bf16x2", "f32x3"])
def test_trunk_plan_is_the_parents_table(shim, arith, two_lanes):
    for frames in FRAMES:
        layers, blocks, dgrad_bf16 = trunk_plan(shim, arith, frames, two_lanes=two_lanes)
        assert layers == TRUNK[(arith, frames)], (arith, frames, layers)
        assert blocks == W1_BLOCKS[two_lanes]
        assert dgrad_bf16 == (arith == BF16X2)  # f32x3 keeps the f32 data-gradient GEMMs


def test_trunk_plan_with_split_multipliers(shim):
    """the multipliers touch the three-part GEMMs only: f32 and bf16x2 keep their table whatever they are"""
    for frames in FRAMES:
        for two_lanes in (False, True):
            assert trunk_plan(shim, F32X3, frames, mul=(2, 2, 2), two_lanes=two_lanes)[0] == TRUNK_X3_MUL2[frames], frames
        for arith in (F32, BF16X2):
            assert trunk_plan(shim, arith, frames, mul=(2, 2, 2))[0] == TRUNK[(arith, frames)], (arith, frames)
            assert trunk_plan(shim, arith, frames, mul=(8, 8, 8))[0] == TRUNK[(arith, frames)], (arith, frames)
    for frames, want in TRUNK_X3_MUL234.items():
        assert trunk_plan(shim, F32X3, frames, mul=(2, 3, 4))[0] == want, frames
    assert trunk_plan(shim, F32X3, 5312, mul=(8, 8, 8))[0] == ((F32X3, 224), (F32X3, 216), (F32X3, 512))


def test_trunk_plan_with_a_lowered_fast_wgrad_min_frames(shim):
    """rela_debug_trunk_backward's override: conv2 / conv3 reach wgrad_conv{2,3}_bf16 from that many frames in bf16x2, and
    nothing else moves"""
    assert trunk_plan(shim, BF16X2, 1, min_frames=3)[0] == ((BF16X2, 84), (BF16X2, 81), KERNEL)
    assert trunk_plan(shim, BF16X2, 2, min_frames=3)[0] == ((BF16X2, 84), (BF16X2, 81), KERNEL)
    for frames in (3, 512, 1024, 1025, 2047, 2048, 5312):
        assert trunk_plan(shim, BF16X2, frames, min_frames=3)[0] == (KERNEL, KERNEL, KERNEL), frames
    assert trunk_plan(shim, BF16X2, 1024, min_frames=1025)[0] == ((BF16X2, 84), (BF16X2, 81), KERNEL)
    assert trunk_plan(shim, BF16X2, 1025, min_frames=1025)[0] == (KERNEL, KERNEL, KERNEL)
    for arith in (F32, F32X3):
        for frames in FRAMES:
            assert trunk_plan(shim, arith, frames, min_frames=3) == trunk_plan(shim, arith, frames), (arith, frames)
            assert trunk_plan(shim, arith, frames, min_frames=3)[0] == TRUNK[(arith, frames)], (arith, frames)


@pytest.mark.parametrize("two_lanes", [False, True], ids=["one-lane", "two-lanes"])
@pytest.mark.parametrize("precision", [0, 1, 2], ids=["f32", "bf16x2", "f32x3"])
def test_apex_plan(shim, precision, two_lanes):
    """heads and fc in the precision's arithmetic; the trunk in the same, multipliers 1, 1, 1"""
    for frames in FRAMES:
        heads_fc, (layers, blocks, dgrad_bf16) = apex_plan(shim, precision, two_lanes, frames)
        assert heads_fc == (F32, BF16X2, F32X3)[precision]
        assert layers == TRUNK[((F32, BF16X2, F32X3)[precision], frames)], (precision, frames)
        assert blocks == W1_BLOCKS[two_lanes] and dgrad_bf16 == (precision == 1)


# precision -> (LSTM input side on rec64, arithmetic of its GEMMs otherwise, the trunk's layers at 1,023 and 1,024 rows and at
# 5,312) -- modes 0 and 2 share a backward; mode 3 has the multipliers 2, 2, 2
R2D2 = {
    0: (False, F32, ((F32, 84), (F32, 81), (F32, 64)), ((F32, 28), (F32, 27), (F32, 64))),
    1: (True, F32, ((BF16X2, 84), (BF16X2, 81), KERNEL), (KERNEL, KERNEL, KERNEL)),
    2: (False, F32, ((F32, 84), (F32, 81), (F32, 64)), ((F32, 28), (F32, 27), (F32, 64))),
    3: (False, F32X3, ((F32X3, 84), (F32X3, 81), (F32X3, 128)), ((F32X3, 56), (F32X3, 54), (F32X3, 128))),
}


@pytest.mark.parametrize("precision", [0, 1, 2, 3], ids=["f32", "bf16x2", "f32x3", "f32x3_bwd"])
def test_r2d2_plan(shim, precision):
    rec64, lstm_in, small, large = R2D2[precision]
    for rows, splits, layers in ((1023, 1, small), (1024, 32, small), (5312, 32, large)):
        head, (got, blocks, dgrad_bf16) = r2d2_plan(shim, precision, rows)
        assert head["heads"] == F32 and head["head_wgrad_splits"] == splits, (precision, rows, head)
        assert head["rec64"] == rec64, (precision, rows)
        if not rec64:  # (on the rec64 path no GEMM of the input side reads the arithmetic)
            assert head["lstm_in"] == lstm_in, (precision, rows)
        assert got == layers, (precision, rows, got)
        assert blocks == 256 and dgrad_bf16 == (precision == 1)  # one lane
