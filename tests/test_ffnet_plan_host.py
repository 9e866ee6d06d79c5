"""Host-logic tests of the forward plan (rela_amd/csrc/ffnet_plan.h): which trunk and which fc a forward of N rows
runs in each precision mode, as the pure function the library calls before it launches anything.

tests/cpu_shims/ffnet_plan_host.cpp puts that header behind a C ABI; the plan is compared with the tables the GPU
tests assert through the launch census (test_ffnet_gpu.expected_kernels, test_learner_gpu's merged-forward table),
imported from there, so the decision is checked wherever g++ exists.  CPU-only.
"""
import ctypes as C
import os
import subprocess

import pytest

import test_ffnet_gpu as ffnet_table
import test_learner_gpu as learner_table
from kernel_names import CONV12, CONV12_JOBS, SPLIT_BF16, X3_FFNET

HERE = os.path.dirname(os.path.abspath(__file__))

NS = [1, 2, 3, 7, 80, 127, 128, 130, 257, 511, 512, 514, 1023, 1024, 1537, 2003, 2047, 2048, 6400, 80000, 80001]
MAX_ROWS = [0, 64, 127, 128, 512, 1023, 1024, 2046]
PRECISIONS = {"f32": 0, "bf16x2": 1, "f32x3": 2}
MODE_NET, MODE_LEARNER_F32X3 = -1, 3
NPOS = 49  # positions of a3 = slices of K the bf16 fc can be cut into

TRUNK_F32, TRUNK_BF16, TRUNK_S3 = 0, 1, 2
FC_F32_SPLITK, FC_F32_GEMM, FC_BF16, FC_BF16_SPLITK, FC_S3, FC_S3_SPLITK = range(6)
# the launch-census names of what each plan value launches (csrc/ffnet.hip: launch_trunk, ffnet_forward_mode)
TRUNK_KERNELS = {TRUNK_F32: {"conv1_bf16x3", "conv_mfma<Conv2> (f32)", "conv_mfma<Conv3> (f32)"},
                 TRUNK_BF16: {CONV12, "conv_bf16s<Conv3F>"},
                 TRUNK_S3: {"conv12_s3", "conv3_img_s3"}}
FC_KERNELS = {FC_F32_SPLITK: {"fc_reduce"}, FC_F32_GEMM: {"gemm_mfma<GemmFc> (f32)"}, FC_BF16: {"fc_bf16s"},
              FC_BF16_SPLITK: {"fc_bf16s (split-K)", "fc_reduce"}, FC_S3: {"gemm_s3<fc>"}, FC_S3_SPLITK: {"gemm_s3<fc>"}}


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "ffnet_plan_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "libffnet_plan_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "ffnet_plan.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


def plan(shim, mode, net_precision, N, max_rows):
    out = (C.c_int * 7)()
    shim.shim_plan_ffnet_forward(mode, net_precision, N, max_rows, out)
    return dict(zip(("trunk", "fc", "keep_f32", "unsplit_a3", "fc_slices", "fc_per", "precision"), out))


def plan_kernels(p):
    k = TRUNK_KERNELS[p["trunk"]] | FC_KERNELS[p["fc"]]
    return k | {"unsplit_records64"} if p["unsplit_a3"] else k


def reachable(N, max_rows):
    """rela_ffnet_forward refuses a batch above the rows its owner declared (max_rows > 0), and the tables of the GPU
    tests describe forwards that run"""
    return max_rows == 0 or N <= max_rows


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_plan_launches_the_kernels_the_gpu_tables_state(shim, precision):
    """Over the kernels the tables speak about (every mode's expected set, the split-bf16 and f32x3 lists of
    kernel_names), the plan launches exactly expected_kernels(N, precision) -- set through the net's own precision
    and through the caller's mode alike."""
    universe = set(SPLIT_BF16) | set(X3_FFNET)
    for N in NS:
        for p in PRECISIONS:
            universe |= ffnet_table.expected_kernels(N, p)
    checked = 0
    for N in NS:
        for max_rows in MAX_ROWS:
            if not reachable(N, max_rows):
                continue
            want = ffnet_table.expected_kernels(N, precision)
            for mode, net_precision in ((MODE_NET, PRECISIONS[precision]), (PRECISIONS[precision], 0),
                                        (PRECISIONS[precision], 1), (PRECISIONS[precision], 2)):
                p = plan(shim, mode, net_precision, N, max_rows)
                assert p["precision"] == PRECISIONS[precision]
                got = plan_kernels(p) & universe
                if precision == "f32x3" and N > 80000:
                    # above kEmuMaxN the records' 32-bit byte offsets end: the f32 kernels, which the table (written for
                    # the batches the GPU tests run) does not know about
                    assert got == ffnet_table.expected_kernels(N, "f32"), (N, max_rows, mode, sorted(got))
                else:
                    assert got == want, (N, max_rows, mode, sorted(got), sorted(want))
                checked += 1
    assert checked >= 4 * len(NS)  # (max_rows = 0 alone reaches every N)


def test_split_k_slices_cover_the_contraction_and_fit_the_partial_tiles(shim):
    split = 0
    for N in NS:
        for max_rows in MAX_ROWS:
            p = plan(shim, MODE_NET, 1, N, max_rows)
            if p["fc"] != FC_BF16_SPLITK:
                assert p["fc_per"] == 0
                continue
            split += 1
            per = C.c_int()
            assert shim.shim_fc_bf16_slices(N, C.byref(per)) == p["fc_slices"] and per.value == p["fc_per"]
            assert p["fc_slices"] * N <= 8192
            assert p["fc_slices"] * p["fc_per"] >= NPOS
            assert (p["fc_slices"] - 1) * p["fc_per"] < NPOS
    assert split > 0
    for N in NS:
        p = plan(shim, MODE_NET, 0, N, 0)
        if p["fc"] == FC_F32_SPLITK:
            assert p["fc_slices"] == shim.shim_fc_splits(N) >= 1 and p["fc_slices"] * N <= 4096
        else:
            assert p["fc"] == FC_F32_GEMM and N >= 2048 and p["fc_slices"] == 1


def test_only_the_learner_mode_keeps_f32(shim):
    for N in NS:
        for max_rows in MAX_ROWS:
            for net_precision in (0, 1, 2):
                for mode in (-1, 0, 1, 2, 3):
                    p = plan(shim, mode, net_precision, N, max_rows)
                    assert p["keep_f32"] == (mode == MODE_LEARNER_F32X3)
                # ... and is the f32x3 arithmetic whatever the net's own precision says
                p3, p2 = plan(shim, MODE_LEARNER_F32X3, net_precision, N, max_rows), plan(shim, 2, net_precision, N, max_rows)
                assert {k: v for k, v in p3.items() if k != "keep_f32"} == {k: v for k, v in p2.items() if k != "keep_f32"}


def test_a_net_packed_for_fewer_rows_never_reads_layouts_it_skipped(shim):
    """rela_ffnet_load skips B2e / B3e below kEmuConvMinN declared rows and Bff below kFastTrunkMinN: whatever N the
    plan is asked about, it must not pick the kernels that read them"""
    for N in NS:
        for max_rows in (64, 127, 128, 511):
            assert plan(shim, MODE_NET, 2, N, max_rows)["trunk"] != TRUNK_S3
            assert plan(shim, MODE_LEARNER_F32X3, 0, N, max_rows)["trunk"] != TRUNK_S3
        for max_rows in (64, 127):
            assert not shim.shim_packs_bf16_fc(max_rows)
            if reachable(N, max_rows):
                assert plan(shim, MODE_NET, 1, N, max_rows)["fc"] not in (FC_BF16, FC_BF16_SPLITK)
    assert shim.shim_packs_bf16_fc(0) and shim.shim_packs_bf16_fc(128)


# ---- which layouts a load packs (ffnet_pack_set) ---------------------------------------------------------------------
FFNET_LAYOUTS = ("B1", "b1", "B2", "b2", "B3", "b3", "Bh", "bh", "W1d", "B2f", "B3f", "B2e", "B3e", "Bf", "BfT", "bf", "Bhp",
                 "Bff", "Bfe")
# What rela_ffnet_load left out at the commit before the pack set became a function, read off the gates of its
# ffnet_load_impl (max_rows > 0 and below: 512 -> B2e, B3e; 512 -> Bfe; 2048 -> Bf; 128 -> Bff), by declared rows ...
PACK_SKIPS = {0: (), 64: ("B2e", "B3e", "Bfe", "Bf", "Bff"), 127: ("B2e", "B3e", "Bfe", "Bf", "Bff"),
              128: ("B2e", "B3e", "Bfe", "Bf"), 511: ("B2e", "B3e", "Bfe", "Bf"), 512: ("Bf",), 2047: ("Bf",), 2048: ()}
# ... and BfT, which a load from device pointers of a split-bf16 net of 128 declared rows and more left to the first
# forward that reads it
LAZY_BFT_ROWS = (128, 511, 512, 2047, 2048)


def _layout_bits(shim):
    rows = (C.c_int * 32)()
    assert shim.shim_ffnet_layouts(rows) == len(FFNET_LAYOUTS)
    assert sorted(rows[:len(FFNET_LAYOUTS)]) == list(range(len(FFNET_LAYOUTS)))
    return {name: 1 << rows[i] for i, name in enumerate(FFNET_LAYOUTS)}


def test_pack_set_is_what_the_load_gates_packed(shim):
    shim.shim_ffnet_pack_set.restype = C.c_uint
    bit = _layout_bits(shim)
    for max_rows, skips in PACK_SKIPS.items():
        for precision in (0, 1, 2):
            for on_device in (0, 1):
                lazy = bool(on_device and precision == 1 and max_rows in LAZY_BFT_ROWS)
                want = set(FFNET_LAYOUTS) - set(skips) - ({"BfT"} if lazy else set())
                got = shim.shim_ffnet_pack_set(max_rows, precision, on_device)
                assert {n for n in FFNET_LAYOUTS if got & bit[n]} == want, (max_rows, precision, on_device)
                assert got == sum(bit[n] for n in want)  # no bits beyond the net's rows
                assert bool(shim.shim_ffnet_bft_on_demand(max_rows, precision, on_device)) == lazy


def test_every_plan_reads_only_layouts_the_load_packed(shim):
    """for every forward that runs (N within the declared rows) in every mode, whatever precision the net had when it
    was loaded: the layouts the plan's kernels read are in the pack set -- or are BfT where the load left it to be
    packed on demand"""
    shim.shim_ffnet_pack_set.restype = shim.shim_ffnet_plan_reads.restype = C.c_uint
    bit = _layout_bits(shim)
    checked = 0
    for N in NS:
        for max_rows in MAX_ROWS + [2047, 2048]:
            if not reachable(N, max_rows):
                continue
            for net_precision in (0, 1, 2):
                for on_device in (0, 1):
                    have = shim.shim_ffnet_pack_set(max_rows, net_precision, on_device)
                    if shim.shim_ffnet_bft_on_demand(max_rows, net_precision, on_device):
                        assert not have & bit["BfT"]
                        have |= bit["BfT"]
                    for mode in (-1, 0, 1, 2, 3):
                        reads = shim.shim_ffnet_plan_reads(mode, net_precision, N, max_rows)
                        assert reads and reads & ~have == 0, (N, max_rows, net_precision, on_device, mode,
                                                              [n for n in FFNET_LAYOUTS if reads & ~have & bit[n]])
                        checked += 1
    assert checked >= 30 * len(NS)
    # the learner's merged f32x3 forward: 2 B rows through a net that declared B, with the limit 2 B handed to the call
    for B in (512, 600, 1024):
        have = shim.shim_ffnet_pack_set(B, 2, 1)
        assert shim.shim_ffnet_plan_reads(MODE_LEARNER_F32X3, 2, 2 * B, 2 * B) & ~have == 0
        p = plan(shim, MODE_LEARNER_F32X3, 2, 2 * B, 2 * B)
        assert p["trunk"] == TRUNK_S3 and p["fc"] == (FC_S3_SPLITK if 2 * B == 1024 else FC_S3)


def test_learner_merged_forward_matches_the_learner_table(shim):
    """test_learner_gpu's statement of which batches the merged split-bf16 forward serves, and what it launches"""
    for B in NS:
        merged = bool(shim.shim_learner_merged_rows(B))
        assert merged == (learner_table.MERGED_MIN_B <= B <= learner_table.MERGED_MAX_B), B
        counts = {"wgrad_conv1_bf16": 1, "dgrad_conv2_bf16": 1, "dgrad_conv3_bf16": 1}
        if merged:
            # online over [s ; s'] (2 B rows) and target over s' (B rows): both fcs are split-K launches of fc_bf16s,
            # whose partial tiles must fit at 2 B rows too
            for rows in (2 * B, B):
                per = C.c_int()
                slices = shim.shim_fc_bf16_slices(rows, C.byref(per))
                assert slices >= 1 and slices * rows <= 8192 and slices * per.value >= NPOS > (slices - 1) * per.value
            counts.update({CONV12_JOBS: 1, "conv3_bf16s_jobs": 1, "fc_bf16s (split-K)": 2, "unsplit_trunk_rows": 1})
        learner_table._assert_fast_learner_kernels(counts, B)


def test_lstm_trunk_plan(shim):
    def lstm(fast, emu, rec, N, want):
        out = (C.c_int * 2)()
        shim.shim_plan_lstm_trunk(fast, emu, rec, N, want, out)
        return out[0], bool(out[1])

    for N in NS:
        for want in (0, 1):
            assert lstm(0, 0, 1, N, want) == (TRUNK_F32, False)
            # split-bf16 from FAST_TRUNK_MIN_N rows; a3 stays in records only where the caller can take them
            assert lstm(1, 0, 1, N, want) == ((TRUNK_BF16, bool(want)) if N >= ffnet_table.FAST_TRUNK_MIN_N else (TRUNK_F32, False))
            # f32x3 needs record scratch as well as EMU_MIN_N <= N <= kEmuMaxN; its a3 always stays in records
            s3 = ffnet_table.EMU_MIN_N <= N <= 80000
            assert lstm(0, 1, 1, N, want) == ((TRUNK_S3, True) if s3 else (TRUNK_F32, False))
            assert lstm(0, 1, 0, N, want) == (TRUNK_F32, False)


def test_mirrored_literals_equal_the_headers_constants(shim):
    c = (C.c_longlong * 9)()
    shim.shim_constants(c)
    fast_min_n, fast_trunk_min_n, emu_conv_min_n, emu_fc_min_n, emu_max_n, fc_split_below, part_floats, part_rows, npos = c
    assert ffnet_table.FAST_TRUNK_MIN_N == fast_trunk_min_n
    assert ffnet_table.FAST_FC_MIN_N == fast_min_n
    assert ffnet_table.EMU_MIN_N == emu_conv_min_n == emu_fc_min_n
    assert learner_table.MERGED_MIN_B == fast_trunk_min_n
    assert learner_table.MERGED_MAX_B == fc_split_below // 2 - 1 == fast_min_n - 1
    assert emu_max_n == 80000 and part_rows == 8192 and part_floats == 8192 * 512 and npos == NPOS
