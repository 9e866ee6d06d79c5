"""conv12_s3_copy (csrc/conv12_s3.h): conv12_s3<false> that also stores every input frame into a ring of frame rows.

The Ape-X shard's target forward writes next_obs into the replay with it (csrc/actor.hip), so two things must hold bit
for bit: what the forward computes is what conv12_s3<false> computes on the same input, and the destination rows are the
input frames.  Through rela_ffnet_debug_forward_store_frames, at 512, 513 and 769 frames (the sizes of
tests/test_conv12_s3_bits_gpu.py: the smallest batch on this path, and batches where only some blocks run a second /
a third round, so both the first-frame store in front of the frame loop and the stores under conv2, the last round's
repeated store included, happen on some blocks and not on others):

  * the a2 records in the workspace (81 x 384 B per frame) and Q equal those of an ordinary rela_ffnet_forward;
  * row (first + i) mod ring of the destination equals frame i byte for byte -- with first = 0 in a ring of exactly n
    rows, and with first = ring - 100 in a ring of n + 37 rows, where the block wraps;
  * the destination buffer is filled with 0xA5 first and has 4,096 guard bytes on either side: the guards and the rows
    of the ring the block does not cover are untouched;
  * the census shows that conv12_s3_copy ran (and did not in the ordinary forward).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 18
FRAME = 4 * 84 * 84
GUARD = 4096
ROWS = (512, 513, 769)


@pytest.fixture(scope="module")
def net():
    import torch

    from rela_amd.engine import FFNetHandle
    from synth import synth_params

    h = FFNetHandle(A, "cuda:0")
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 51).items()})
    h.set_precision("f32x3")
    yield h
    h.close()


def _forward(net, frames, store=None):
    """-> (Q, a2 records, census[, destination buffer with its guards]); store = (first, ring)"""
    import torch

    from rela_amd import _capi as capi

    n = frames.shape[0]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    legal = torch.ones((n, A), device="cuda")
    q = torch.empty((n, A), device="cuda")
    nb = capi.lib.rela_ffnet_workspace_bytes(net.h, n)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    view = capi.DebugWorkspaceView()
    capi.check(capi.lib.rela_ffnet_debug_workspace(net.h, n, C.byref(view)), "debug_workspace")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dst = None
    with capi.launch_census() as census:
        if store is None:
            capi.check(capi.lib.rela_ffnet_forward(net.h, n, ptr(frames), ptr(legal), ptr(q), ptr(ws), nb, stream), "forward")
        else:
            first, ring = store
            dst = torch.full((2 * GUARD + ring * FRAME,), 0xA5, dtype=torch.uint8, device="cuda")
            copied = C.c_int(0)
            capi.check(capi.lib.rela_ffnet_debug_forward_store_frames(
                net.h, n, ptr(frames), ptr(legal), ptr(q), ptr(ws), nb, C.c_void_p(dst.data_ptr() + GUARD), first, ring,
                C.byref(copied), stream), "forward_store_frames")
            assert copied.value == 1
        torch.cuda.synchronize()
    rec2 = ws[view.rec2:view.rec2 + n * 81 * 384].cpu().numpy()
    return q.cpu().numpy(), rec2, dict(census.counts), (dst.cpu().numpy() if dst is not None else None)


@pytest.mark.parametrize("n", ROWS)
def test_copy_variant_keeps_the_bits_and_stores_the_frames(net, n):
    import torch

    from synth import synth_obs

    host = synth_obs(n, 7000 + n)
    frames = torch.from_numpy(host).cuda()
    flat = host.reshape(n, FRAME)
    q0, rec0, ran0, _ = _forward(net, frames)
    assert ran0.get("conv12_s3") == 1 and "conv12_s3_copy" not in ran0, ran0
    assert rec0.any()
    for first, ring in ((0, n), (n + 37 - 100, n + 37)):
        q1, rec1, ran1, dst = _forward(net, frames, (first, ring))
        assert ran1.get("conv12_s3_copy") == 1 and ran1.get("conv12_s3") == 1, ran1
        assert np.array_equal(rec1, rec0), "a2 records differ from conv12_s3<false>"
        assert np.array_equal(q1.view(np.uint32), q0.view(np.uint32))
        assert (dst[:GUARD] == 0xA5).all() and (dst[-GUARD:] == 0xA5).all(), "guard bytes written"
        rows = dst[GUARD:-GUARD].reshape(ring, FRAME)
        slots = (first + np.arange(n)) % ring
        assert np.array_equal(rows[slots], flat), "destination rows are not the input frames"
        rest = np.setdiff1d(np.arange(ring), slots)
        assert rest.size == ring - n and (rows[rest] == 0xA5).all(), "rows outside the block written"


def test_other_trunks_report_that_they_did_not_copy(net):
    """Below 512 rows the f32x3 net's trunk is not conv12_s3: the forward runs as usual, says so, and writes nothing."""
    import torch

    from rela_amd import _capi as capi
    from synth import synth_obs

    n = 128
    frames = torch.from_numpy(synth_obs(n, 7000)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    legal = torch.ones((n, A), device="cuda")
    q, q_ref = torch.empty((n, A), device="cuda"), torch.empty((n, A), device="cuda")
    nb = capi.lib.rela_ffnet_workspace_bytes(net.h, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dst = torch.full((n * FRAME,), 0xA5, dtype=torch.uint8, device="cuda")
    copied = C.c_int(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(capi.lib.rela_ffnet_debug_forward_store_frames(net.h, n, ptr(frames), ptr(legal), ptr(q), ptr(ws), nb, ptr(dst), 0, n,
                                                              C.byref(copied), stream), "forward_store_frames")
    capi.check(capi.lib.rela_ffnet_forward(net.h, n, ptr(frames), ptr(legal), ptr(q_ref), ptr(ws), nb, stream), "forward")
    torch.cuda.synchronize()
    assert copied.value == 0
    assert bool((dst == 0xA5).all())
    assert torch.equal(q, q_ref)
