"""Every kernel-layout weight copy of a loaded net holds the SAME BYTES as at the commit before the pack rewrite.

rela_ffnet_load / rela_lstmnet_load fill their layouts with one launch of the weight-pack kernel (csrc/weight_pack.h)
over a list of segments built from the layout table (csrc/ffnet.hip).  Before that the AtariFFNet had a kernel with one
named pointer per layout and the AtariLSTMNet thirteen separate pack kernels and three copies.  The fixture
tests/golden/weight_pack_parent_bits.json holds, per case, the name, size and CRC32 of every layout as that older code
packed it: recorded on an MI355X from a checkout of the commit named in it, through a throwaway patch (never committed)
that added the same readback (rela_*_debug_layout) to it, with this file's `layouts()`.

Inputs come from numpy (tests/synth.py), so they are the same bits everywhere, with conv1's output channel 5 all zeros:
its int8 scale takes the `mx == 0` branch of the conv1 pack.  Cases: num_action 1, 18 and 31 for both nets (31 puts
fc_a's last column next to fc_v's column 31 of the head layouts), and one load per net from HOST pointers
(params_on_device = 0), whose bytes must also equal the load from device pointers of the same run.  The nets declare no
row limit, so every layout is packed; which layouts a limited net packs is checked on the CPU
(tests/test_ffnet_plan_host.py) and what it then computes by the learner tests.

Re-recording (only ever from the commit BEFORE a change to the packing):  python tests/test_weight_pack_bits_gpu.py OUT.json COMMIT
"""
import ctypes as C
import functools
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "weight_pack_parent_bits.json")
ACTIONS = (1, 18, 31)
ZERO_CHANNEL = 5
KINDS = ("ffnet", "lstmnet")


def _params(kind, A):
    from synth import synth_lstm_params, synth_params

    p = synth_params(A, 300 + A) if kind == "ffnet" else synth_lstm_params(A, 400 + A)
    p["net.0.weight"][ZERO_CHANNEL] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def layouts(kind, A, on_device):
    """((name, bytes, crc32), ...) of every layout of a freshly loaded net, through the C ABI alone"""
    import torch

    from rela_amd import _capi as capi

    lib = capi.lib
    struct = capi.FFNetParams if kind == "ffnet" else capi.LSTMNetParams
    fn = lambda what: getattr(lib, "rela_%s_%s" % (kind, what))
    host = [np.ascontiguousarray(v, np.float32) for v in _params(kind, A).values()]
    dev = [torch.from_numpy(v).cuda() for v in host] if on_device else None
    p = struct()
    for (field, _), h, i in zip(struct._fields_, host, range(len(host))):
        setattr(p, field, dev[i].data_ptr() if on_device else h.ctypes.data)
    net = C.c_void_p()
    capi.check(fn("create")(C.byref(net), A, 0), "create")
    try:
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capi.check(fn("load")(net, C.byref(p), 1 if on_device else 0, stream), "load")
        torch.cuda.synchronize()
        out = []
        for index in range(64):
            name, nbytes, packed = C.c_char_p(), C.c_int64(), C.c_int()
            rc = fn("debug_layout")(net, index, C.byref(name), C.byref(nbytes), C.byref(packed), None)
            if rc == capi.EINVAL:  # past the last row of the table
                break
            capi.check(rc, "debug_layout")
            assert packed.value == 1, "%s: a net without a row limit packs every layout" % name.value
            buf = np.full(nbytes.value, 0xA5, np.uint8)
            capi.check(fn("debug_layout")(net, index, None, None, None, C.c_void_p(buf.ctypes.data)), "debug_layout")
            out.append((name.value.decode(), int(nbytes.value), zlib.crc32(buf.tobytes())))
        assert out and index < 63
        return tuple(out)
    finally:
        fn("destroy")(net)


def _golden(kind, A):
    with open(FIXTURE) as f:
        return tuple(tuple(row) for row in json.load(f)["layouts"]["%s_A%d" % (kind, A)])


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_layout_bytes_equal_parent(kind, A):
    got = layouts(kind, A, True)
    want = _golden(kind, A)
    for g in got:
        print(kind, A, *g)
    assert [g[:2] for g in got] == [w[:2] for w in want]  # the same layouts, in the same sizes
    assert got == want


@pytest.mark.parametrize("kind", KINDS)
def test_load_from_host_pointers(kind):
    got = layouts(kind, 18, False)
    assert got == _golden(kind, 18)
    assert got == layouts(kind, 18, True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    rec = {}
    for kind in KINDS:
        for A in ACTIONS:
            rec["%s_A%d" % (kind, A)] = layouts(kind, A, True)
        assert layouts(kind, 18, False) == layouts(kind, 18, True), "host and device loads differ"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "[name, bytes, crc32] of every kernel-layout weight copy after a load (tests/test_weight_pack_bits_gpu.py)",
           "layouts": rec}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc))
