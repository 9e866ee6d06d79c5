"""The issue schedule of gemm_s3's k-loop, read from the compiler's assembly (no GPU needed).

csrc/gemm_s3.h spreads the LDS-DMA pieces of a pair of k-steps (the next pair's activation lines, two k-steps of this
wave's weight fragments) over the pair's MFMA groups instead of issuing them in one burst behind the pair's barrier, and
its comments state what the loop looks like.  This test compiles csrc/ffnet.hip device-only to assembly with build.py's
HIP_FLAGS (about half a minute) and checks, for every instantiation of s3::gemm_s3 and every pair loop in it (one per
pass size 1..7, reached from the kernel's `switch`, in the two forms "the block's larger pass" and "one tile fewer"):

  * exactly one s_barrier per iteration;
  * no `s_waitcnt vmcnt(0)` inside the loop (every wait is counted; the one vmcnt(0) of the kernel is behind the loops);
  * between MFMAs a wave issues at most kMaxGldsRun = 2 global_load_lds_dwordx4 in a row (the constant of
    csrc/gemm_s3.h, read from the header so that the two cannot drift apart), also across the loop's back edge.

A pair loop is an innermost loop (a backward branch to a label, with no other backward branch inside its range) that
holds MFMAs and a barrier.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_SIZES = 7  # TMV of csrc/gemm_s3.h


def _max_run_constant():
    with open(os.path.join(ROOT, "rela_amd", "csrc", "gemm_s3.h")) as f:
        m = re.search(r"constexpr int kMaxGldsRun = (\d+);", f.read())
    assert m, "kMaxGldsRun not found in gemm_s3.h"
    return int(m.group(1))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: [instruction lines]} of csrc/ffnet.hip's gemm_s3 kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    asm = str(tmp_path_factory.mktemp("s3sched") / "ffnet_dev.s")
    cmd = [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "ffnet.hip"), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    name = None
    with open(asm) as f:
        for line in f:
            line = line.split(";")[0].rstrip()
            m = re.match(r"^(_ZN8rela_amd2s37gemm_s3I\w+):", line)
            if m:
                name = m.group(1)
                out[name] = []
                continue
            if name is None or not line.strip():
                continue
            if line.startswith(".Lfunc_end"):
                name = None
                continue
            out[name].append(line.strip())
    return out


def pair_loops(lines):
    """innermost loops (lists of lines, label to backward branch) that hold MFMAs and a barrier"""
    label_at = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
    spans = []
    for i, l in enumerate(lines):
        m = re.match(r"^s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            spans.append((label_at[m.group(1)], i))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    loops = [lines[a:b + 1] for a, b in inner]
    return [lp for lp in loops if any(l.startswith("v_mfma") for l in lp) and any(l.startswith("s_barrier") for l in lp)]


def longest_glds_run(loop):
    """most global_load_lds_dwordx4 in a row with no MFMA between them, the back edge included"""
    ops = [l for l in loop if l.startswith("v_mfma") or l.startswith("global_load_lds_dwordx4")]
    assert any(l.startswith("v_mfma") for l in ops)
    best = run = 0
    for l in ops + ops:  # (twice: a run may wrap around the back edge)
        run = run + 1 if l.startswith("global_load_lds") else 0
        best = max(best, run)
    return best


def test_every_instantiation_has_its_pair_loops(kernels):
    # fc (ReLU; raw sums for split-K) and the gate GEMM (raw sums; bias): the four instantiations ffnet.hip launches
    assert len(kernels) >= 4, sorted(kernels)
    for name, lines in kernels.items():
        loops = pair_loops(lines)
        # pass sizes 1..7 as the block's larger pass, 1..6 as the smaller one
        assert len(loops) >= 2 * PASS_SIZES - 1, (name, len(loops))
        for lp in loops:
            assert any(l.startswith("global_load_lds_dwordx4") for l in lp), name


def test_one_barrier_per_pair(kernels):
    for name, lines in kernels.items():
        for lp in pair_loops(lines):
            assert sum(l.startswith("s_barrier") for l in lp) == 1, (name, lp[0])


def test_no_vmcnt0_in_the_pair_loop(kernels):
    for name, lines in kernels.items():
        for lp in pair_loops(lines):
            waits = [l for l in lp if l.startswith("s_waitcnt") and "vmcnt" in l]
            assert waits, (name, lp[0])  # the counted waits are there
            bad = [l for l in waits if re.search(r"vmcnt\(0\)", l)]
            assert not bad, (name, lp[0], bad)


def test_glds_runs_between_mfmas_are_bounded(kernels):
    bound = _max_run_constant()
    assert bound in (1, 2)
    for name, lines in kernels.items():
        runs = [longest_glds_run(lp) for lp in pair_loops(lines)]
        print(name, runs)
        assert max(runs) <= bound, (name, runs)
