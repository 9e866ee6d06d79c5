"""Every learner kernel is compiled once: no kernel of csrc/learner.hip, csrc/learner_r2d2.hip and csrc/learner_common.hip
occurs in two of them.

What the Ape-X and the R2D2 learner share -- the conv trunk's backward pass, column sums, the heads' weight gradient, the
optimisers -- lives in learner_common.hip behind launchers (learner_common.h), so that the per-call test taps run the very
code both learners run.  A kernel that slips back into a header both learners include would be compiled per unit again, and
the taps would see one copy of it only.  So the three units are compiled device-only with build.py's HIP_FLAGS plus
-Rpass-analysis=kernel-resource-usage (tests/kernel_resources.py, no GPU needed) and the kernel names of the remarks are
compared, with the suffix a compiler may give to names of internal linkage taken off.  The one exception is
dev_copy2_kernel: `static` in common.h, it reaches every unit that copies.  Only the kernel names are read.
"""
import os
import re
import subprocess

import pytest

from kernel_resources import device_only_cmd, parse_remarks

UNITS = ("learner.hip", "learner_r2d2.hip", "learner_common.hip")
SHARED_ON_PURPOSE = "16dev_copy2_kernelE"  # substring of the mangled name
INTERNAL_SUFFIX = re.compile(r"(\.(static|intern|uniq|llvm)\.\w+|__uniq\w*)$")
# one kernel that each unit owns (substrings of the mangled names), so that an empty or misread listing cannot pass
OWN = {"learner.hip": "20learner_td_loss_grad", "learner_r2d2.hip": "17head_wgrad_reduce", "learner_common.hip": "13reduce_splits"}


@pytest.fixture(scope="module")
def kernel_names(tmp_path_factory):
    """{unit: set of its kernels' mangled names without internal-linkage suffix}"""
    tmp = tmp_path_factory.mktemp("learner_units")
    jobs = {u: subprocess.Popen(device_only_cmd(u, os.path.join(str(tmp), u[:-4] + "_dev.o")), stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True) for u in UNITS}
    out = {}
    for u, proc in jobs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-4000:]
        out[u] = {INTERNAL_SUFFIX.sub("", n) for n in parse_remarks(err)}
    return out


def test_internal_suffix_is_taken_off():
    for name in ("_ZN8rela_amd12_GLOBAL__N_113reduce_splitsEPKfiiiiPf", "_ZN8rela_amdL16dev_copy2_kernelEPhPKhmS0_S2_m"):
        for suffix in ("", ".static.1a2b3c", ".intern.5f", "__uniq123", ".llvm.987"):
            assert INTERNAL_SUFFIX.sub("", name + suffix) == name


@pytest.mark.parametrize("unit", UNITS)
def test_each_unit_holds_its_own_kernels(kernel_names, unit):
    assert any(OWN[unit] in n for n in kernel_names[unit]), sorted(kernel_names[unit])
    for other in UNITS:
        if other != unit:
            assert not any(OWN[unit] in n for n in kernel_names[other]), (other, OWN[unit])


def test_no_kernel_is_compiled_in_two_units(kernel_names):
    twice = sorted(n for i, a in enumerate(UNITS) for b in UNITS[i + 1:] for n in kernel_names[a] & kernel_names[b])
    print({u: len(v) for u, v in kernel_names.items()}, twice)
    assert [n for n in twice if SHARED_ON_PURPOSE not in n] == [], twice
