"""The chunk loops of the learner's GEMMs keep their load ring in flight: read from the compiled code, no GPU needed.

csrc/gemm_lds.h and csrc/gemm_bf16x3.h hold D chunks of operands in a register ring (gemm::chunk_ring) so that no chunk
waits out its own loads.  That only works while hipcc can COUNT the loads: a loader that decides `in range ? load : zero`
is compiled to a branch around the load (s_cbranch_execz), the compiler cannot count across the join and every wait in
the loop becomes `s_waitcnt vmcnt(0)` -- the ring then holds nothing but the loads of the current step, and no test of
the results notices.  The loader contract (gemm_lds.h: fetch from a clamped address, fix up with a select at the store)
removes the branches; this file asserts what the compiler made of it.

csrc/learner.hip, csrc/learner_r2d2.hip and csrc/learner_common.hip are compiled device-only to assembly with build.py's HIP_FLAGS plus
-Rpass-analysis=kernel-resource-usage, and for EVERY gemm_bf16x3 / gemm_lds function in them:
  * inside the blocks the compiler marks as part of the chunk loop there is a loop at all, with global loads in it;
  * none of those blocks ends in a branch on EXEC (no load sits behind a per-lane condition);
  * none of them holds `s_waitcnt vmcnt(0)`;
  * at least one wait there is counted with N >= the global loads of one chunk (loads in the loop / barriers in the
    loop: a step refills one chunk and ends in one barrier), i.e. it leaves a later chunk outstanding;
  * the resource remarks say no scratch and no spills.
Only `s_waitcnt vmcnt`, loads, branches, barriers and the resource remarks are read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("learner.hip", "learner_r2d2.hip", "learner_common.hip")
FAMILIES = ("11gemm_bf16x3I", "8gemm_ldsI")  # substrings of the mangled names of the two kernel templates
# kernels that must be there (substrings of the mangled name), so that an empty match cannot pass; the conv trunk's and the
# heads' weight gradient of both learners are compiled in learner_common.hip alone
EXPECTED = {"learner.hip": [("11gemm_bf16x3I", "11ProbFcWgradE"), ("11gemm_bf16x3I", "11ProbFcDgradE"),
                            ("11gemm_bf16x3I", "13ProbHeadDgradE")],
            "learner_r2d2.hip": [("8gemm_ldsI", "9ProbGateXE"), ("8gemm_ldsI", "10ProbRecFwdE"),
                                 ("8gemm_ldsI", "10ProbRecBwdE"), ("8gemm_ldsI", "7ProbWhhE"), ("8gemm_ldsI", "7ProbWihE"),
                                 ("8gemm_ldsI", "11ProbIhDgradE"), ("8gemm_ldsI", "16ProbHeadDgradSeqE")],
            "learner_common.hip": [("11gemm_bf16x3I", "11SinglePartBI", "6ProbW1E"), ("8gemm_ldsI", "10ProbDgrad3E"),
                                   ("8gemm_ldsI", "10ProbDgrad2E"), ("11gemm_bf16x3I", "13ProbHeadWgradE"),
                                   ("11gemm_bf16x3I", "13ProbConvWgradI")]}


def parse_remarks(stderr):
    """-> {mangled kernel name: {remark key: int}}"""
    out, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def parse_loops(asm):
    """-> {function name: {"blocks", "loads", "barriers", "exec_branches", "waits": [N of every vmcnt wait]}} counted over
    the basic blocks that the compiler's comments put inside a loop (`Loop Header`, `in Loop:`, `Parent Loop`)"""
    out, name, in_loop = {}, None, False
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, in_loop = m.group(1), False
            out[name] = {"blocks": 0, "loads": 0, "barriers": 0, "exec_branches": 0, "waits": []}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            in_loop = "Loop" in line
            out[name]["blocks"] += in_loop
            continue
        if not in_loop:
            continue
        ins = line.strip()
        f = out[name]
        if re.match(r"(global|buffer|flat)_load", ins):
            f["loads"] += 1
        elif ins.startswith("s_barrier"):
            f["barriers"] += 1
        elif re.match(r"s_cbranch_exec", ins):
            f["exec_branches"] += 1
        else:
            m = re.match(r"s_waitcnt\b.*vmcnt\((\d+)\)", ins)
            if m:
                f["waits"].append(int(m.group(1)))
    return out


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{source: ({kernel: loop facts}, {kernel: resource remarks})} of the gemm_bf16x3 / gemm_lds kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    tmp = tmp_path_factory.mktemp("gemmwaits")
    jobs = {}
    for src in SOURCES:
        asm = str(tmp / (src[:-4] + ".s"))
        cmd = [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                                       os.path.join(b.CSRC, src), "-o", asm]
        jobs[src] = (asm, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for src, (asm, proc) in jobs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-4000:]
        with open(asm) as f:
            loops = parse_loops(f.read())
        mine = lambda d: {n: v for n, v in d.items() if any(fam in n for fam in FAMILIES)}
        out[src] = (mine(loops), mine(parse_remarks(err)))
    return out


@pytest.mark.parametrize("src", SOURCES)
def test_every_instantiation_is_found(compiled, src):
    loops, remarks = compiled[src]
    assert set(loops) == set(remarks) and loops
    for parts in EXPECTED[src]:
        assert any(all(p in n for p in parts) for n in loops), (parts, sorted(loops))


@pytest.mark.parametrize("src", SOURCES)
def test_chunk_loops_keep_later_chunks_outstanding(compiled, src):
    bad = []
    for name, f in sorted(compiled[src][0].items()):
        print(name, f)
        if not (f["blocks"] and f["loads"] and f["barriers"]):
            bad.append((name, "no chunk loop with loads and barriers found", f))
            continue
        if f["exec_branches"]:
            bad.append((name, "a branch on EXEC inside the chunk loop", f))
        if 0 in f["waits"]:
            bad.append((name, "s_waitcnt vmcnt(0) inside the chunk loop", f))
        if f["loads"] % f["barriers"]:
            bad.append((name, "loads in the loop are no multiple of its steps", f))
        chunk_loads = f["loads"] // f["barriers"]
        if not any(n >= chunk_loads for n in f["waits"]):
            bad.append((name, "no counted wait leaves a chunk (%d loads) outstanding" % chunk_loads, f))
    assert not bad, bad


@pytest.mark.parametrize("src", SOURCES)
def test_no_scratch_no_spills(compiled, src):
    for name, v in sorted(compiled[src][1].items()):
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)


def test_parser_sees_a_drained_loop():
    """the checks can fail: a loop as the old loaders compiled -- a load behind an EXEC branch, vmcnt(0) at its use"""
    asm = "\n".join(["_Z4demov:", "; %bb.0:", "\tglobal_load_dwordx4 v[0:3], v[4:5], off",
                     ".LBB0_1:                ; =>This Inner Loop Header: Depth=1", "\ts_cbranch_execz .LBB0_3",
                     "; %bb.2:                ;   in Loop: Header=BB0_1 Depth=1",
                     "\tglobal_load_dwordx4 v[0:3], v[4:5], off",
                     ".LBB0_3:                ;   in Loop: Header=BB0_1 Depth=1", "\ts_waitcnt vmcnt(0)",
                     "\ts_waitcnt vmcnt(2) lgkmcnt(0)", "\ts_barrier", "\ts_cbranch_scc1 .LBB0_1", "; %bb.4:",
                     "\ts_waitcnt vmcnt(0)", "\ts_endpgm", ".Lfunc_end0:"])
    f = parse_loops(asm)["_Z4demov"]
    assert f == {"blocks": 3, "loads": 1, "barriers": 1, "exec_branches": 1, "waits": [0, 2]}
