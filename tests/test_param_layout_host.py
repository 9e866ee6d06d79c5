"""The parameter tables of the two nets exist once in C++ (rela_amd/csrc/param_layout.h: the nets' loads and both
learners) and once in Python (rela_amd/learner.py: SHAPES and the flat layouts, with which actor-only ranks cut up the
flat buffer they receive across processes).  These tests hold the two together.

tests/cpu_shims/param_layout_host.cpp puts the header behind a C ABI.  CPU-only.
"""
import ctypes as C
import math
import os
import subprocess

import pytest

from rela_amd.learner import HipApexLearner, HipR2D2Learner, ffnet_flat_layout, lstmnet_flat_layout

HERE = os.path.dirname(os.path.abspath(__file__))

# 1 and 31 are the limits of the learners' create; none is a multiple of 4, so fc_a.bias (A floats) needs padding,
# and fc_v.bias (1 float) always does
ACTIONS = [1, 3, 6, 18, 31]
NETS = {"ffnet": (0, HipApexLearner, ffnet_flat_layout), "lstmnet": (1, HipR2D2Learner, lstmnet_flat_layout)}


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "cpu_shims", "param_layout_host.cpp")
    so = os.path.join(HERE, "cpu_shims", "libparam_layout_host.so")
    hdr = os.path.join(HERE, "..", "rela_amd", "csrc", "param_layout.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


def native_layout(shim, net, A):
    cnt, off = (C.c_longlong * 14)(), (C.c_longlong * 15)()
    nseg = shim.shim_param_layout(net, A, cnt, off)
    return list(cnt[:nseg]), list(off[:nseg + 1])


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("name", sorted(NETS))
def test_native_counts_and_offsets_equal_the_python_layout(shim, name, A):
    net, cls, flat_layout = NETS[name]
    cnt, off = native_layout(shim, net, A)
    shapes = cls.SHAPES(A)
    assert len(cnt) == len(cls.KEYS) == len(shapes)
    assert cnt == [math.prod(s) for s in shapes]
    layout, total = flat_layout(A)
    assert [k for k, _, _ in layout] == list(cls.KEYS) and [s for _, s, _ in layout] == list(shapes)
    assert off[:-1] == [o for _, _, o in layout]
    assert off[-1] == total
    # every tensor starts 16-byte aligned, right behind the one before it padded to 4 floats
    assert off[0] == 0
    for i, n in enumerate(cnt):
        assert off[i] % 4 == 0 and off[i + 1] - off[i] == (n + 3) // 4 * 4
    assert (A + 3) // 4 * 4 > A and off[-1] > sum(cnt)  # these action counts do exercise the padding


def test_ffnet_has_the_parameter_count_the_learner_docstring_states(shim):
    """1,693,875 floats for AtariFFNet at A = 18 (rela_amd/learner.py): the sum before padding."""
    cnt, off = native_layout(shim, 0, 18)
    assert sum(cnt) == 1693875
    assert sum(math.prod(s) for s in HipApexLearner.SHAPES(18)) == 1693875
    assert off[-1] == ffnet_flat_layout(18)[1] >= 1693875
