"""The learner GEMMs that run a deeper stage multiply S chunks per barrier: read from the compiled code, no GPU needed.

csrc/gemm_lds.h and csrc/gemm_bf16x3.h stage S chunks of 32 k per barrier (TileCfg's S).  Two instantiations are built
with S > 1 (csrc/learner_common.hip: conv1's weight gradient -- TileW1, f32, S = 4, and Tile6W32U8, f32x3, S = 2, which
leaves room for a second block on the CU); every other one stays at S = 1.  Per barrier and per wave the chunk loop of an S = 1 kernel holds TM x TN x 8 MFMAs in gemm_lds
(v_mfma_f32_16x16x4_f32, eight k-steps of 4) and TM x TN x (products per step) in gemm_bf16x3 (v_mfma_f32_16x16x32_bf16,
one k-step of 32; 3 products for the one-part B operand of conv1): 8 and 3 for the 32 x 64 tile of conv1 (TM = TN = 1).
With S = 4 / S = 2 the same loops must hold 32 and 6 -- the parent's count times S: a stage that lost a chunk, or a loop that
was not unrolled over the stage, shows here and nowhere in the results' values at full slices.

csrc/learner.hip, csrc/learner_r2d2.hip and csrc/learner_common.hip are compiled device-only to assembly with build.py's
HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage, as tests/test_learner_gemm_waits_cpu.py does; the two staged kernels
are compiled once, in learner_common.hip, for both learners.  Only MFMA and barrier counts inside
the blocks the compiler marks as a loop, and the resource remarks, are read.
"""
import re
import subprocess

import pytest

from kernel_resources import device_only_cmd, parse_remarks

SOURCES = ("learner.hip", "learner_r2d2.hip", "learner_common.hip")
STAGED_IN = "learner_common.hip"  # the unit of the conv trunk's backward pass: the one copy both learners launch
# (substrings of the mangled name) -> (S, MFMAs per barrier of the S = 1 kernel)
STAGED = {("8gemm_ldsI", "6ProbW1E"): (4, 8), ("11gemm_bf16x3I", "11SinglePartBI", "6ProbW1E"): (2, 3)}
# the stage depth is TileCfg's last template argument: ..., true, S> for gemm_lds, ..., true, 3 parts, S> for gemm_bf16x3
STAGE_ARG = {"8gemm_ldsI": r"Lb[01]ELi%dEE", "11gemm_bf16x3I": r"Lb[01]ELi\dELi%dEE"}


def parse_loops(asm):
    """-> {function name: {"mfma", "barriers"}} counted over the basic blocks that the compiler's comments put inside a
    loop (`Loop Header`, `in Loop:`, `Parent Loop`)"""
    out, name, in_loop = {}, None, False
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, in_loop = m.group(1), False
            out[name] = {"mfma": 0, "barriers": 0}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            in_loop = "Loop" in line
            continue
        if not in_loop:
            continue
        ins = line.strip()
        if ins.startswith("v_mfma"):
            out[name]["mfma"] += 1
        elif ins.startswith("s_barrier"):
            out[name]["barriers"] += 1
    return out


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{source: ({kernel: loop counts}, {kernel: resource remarks})} of the gemm_bf16x3 / gemm_lds kernels"""
    tmp = tmp_path_factory.mktemp("gemmstage")
    jobs = {}
    for src in SOURCES:
        asm = str(tmp / (src[:-4] + ".s"))
        jobs[src] = (asm, subprocess.Popen(device_only_cmd(src, asm, "-S"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                           text=True))
    out = {}
    for src, (asm, proc) in jobs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-4000:]
        with open(asm) as f:
            loops = parse_loops(f.read())
        mine = lambda d: {n: v for n, v in d.items() if "11gemm_bf16x3I" in n or "8gemm_ldsI" in n}
        out[src] = (mine(loops), mine(parse_remarks(err)))
    return out


def _find(names, parts):
    return [n for n in names if all(p in n for p in parts) and (parts[0] != "8gemm_ldsI" or "11SinglePartBI" not in n)]


@pytest.mark.parametrize("src", [STAGED_IN])
@pytest.mark.parametrize("parts", sorted(STAGED), ids=["-".join(p) for p in sorted(STAGED)])
def test_staged_loops_hold_s_times_the_mfmas_per_barrier(compiled, src, parts):
    loops, remarks = compiled[src]
    S, per_chunk = STAGED[parts]
    found = _find(loops, parts)
    assert len(found) == 1, (parts, found)
    name = found[0]
    assert re.search(STAGE_ARG[parts[0]] % S, name), name  # built with the stage depth this file expects
    f = loops[name]
    print(name, f, remarks[name])
    assert f["barriers"] > 0 and f["mfma"] % f["barriers"] == 0, f
    assert f["mfma"] // f["barriers"] == S * per_chunk, f
    r = remarks[name]
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    # a block is eight waves, two per SIMD
    assert r["Occupancy [waves/SIMD]"] >= 2, r


@pytest.mark.parametrize("src", SOURCES)
def test_no_other_instantiation_is_staged(compiled, src):
    """whoever gives another tile a stage depth adds it to STAGED, with its measurement in the write-up"""
    loops, _ = compiled[src]
    assert loops
    staged = {n for parts in STAGED for n in _find(loops, parts)} if src == STAGED_IN else set()
    for name in loops:
        fam = "8gemm_ldsI" if "8gemm_ldsI" in name else "11gemm_bf16x3I"
        deep = any(re.search(STAGE_ARG[fam] % s, name) for s in (2, 4))
        assert deep == (name in staged), name


def test_parser_counts_a_staged_loop():
    asm = "\n".join(["_Z4demov:", "; %bb.0:", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]",
                     ".LBB0_1:                ; =>This Inner Loop Header: Depth=1"] +
                    ["\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]"] * 12 +
                    ["\ts_barrier", "\ts_cbranch_scc1 .LBB0_1", "; %bb.2:", "\ts_barrier", "\ts_endpgm", ".Lfunc_end0:"])
    assert parse_loops(asm)["_Z4demov"] == {"mfma": 12, "barriers": 1}
