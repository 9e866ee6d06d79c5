"""What the compiler says about a source file's kernels, without a GPU: the file is compiled device-only with build.py's
HIP_FLAGS plus -Rpass-analysis=kernel-resource-usage, and the remarks are parsed into {mangled kernel name: {remark key:
int}}.  Shared by the CPU tests that assert registers, scratch, LDS and occupancy of the learners' kernels."""
import os
import re
import shutil
import subprocess

import pytest


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


def device_only_cmd(src, out, emit="-c"):
    """the hipcc line that compiles csrc/`src` device-only into `out` (emit: -c object, -S assembly) with the resource
    remarks on stderr; skips the calling test where there is no hipcc"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    return [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", emit,
                                    os.path.join(b.CSRC, src), "-o", out]


def kernel_resources(src, tmp_dir):
    """{mangled kernel name: {remark key: int}} of csrc/`src`'s kernels"""
    r = subprocess.run(device_only_cmd(src, os.path.join(str(tmp_dir), src[:-4] + "_dev.o")), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return parse_remarks(r.stderr)
