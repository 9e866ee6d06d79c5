"""conv12_s3_copy2 (csrc/conv12_s3.h): conv12_s3_copy that also passes a second set of frames through to a second ring.

The Ape-X shard's target forward writes next_obs AND obs into the replay with it (csrc/actor.hip, fused insert 2): the
forward's own input goes to the first ring from the registers it is staged in, as in conv12_s3_copy, and the frames of
a second source, which take no part in the arithmetic, are loaded and stored under the MFMAs.  Through
rela_ffnet_debug_forward_store_frames2, at the row counts of tests/test_conv12_copy_bits_gpu.py (512 and 513 are the
smallest on this path, 513 gives blocks one and two frames, 769 two and three: the pass-through runs in every round):

  * Q and the a2 / a3 records in the workspace equal those of an ordinary rela_ffnet_forward on the same frames;
  * row (first + i) mod ring of the first destination equals input frame i, row (first2 + i) mod ring of the second
    equals frame i of the second source, byte for byte.  The two sources are different random frames, so a mix-up of
    sources or destinations shows; first != first2, and each makes its block wrap its ring (n + 37 rows);
  * both destinations are filled with 0xA5 first; each has one guard row after the ring (and one before it): the guards
    and the ring's rows outside the block are untouched;
  * the census names conv12_s3_copy2 and not conv12_s3_copy;
  * another trunk (an f32 net, a bf16x2 net, an f32x3 net below 512 rows) reports 0 fields and writes nothing.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 18
FRAME = 4 * 84 * 84
ROWS = (512, 513, 769)
EXTRA = 37


def _net(precision, seed=51):
    import torch

    from rela_amd.engine import FFNetHandle
    from synth import synth_params

    h = FFNetHandle(A, "cuda:0")
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, seed).items()})
    h.set_precision(precision)
    return h


@pytest.fixture(scope="module")
def net():
    h = _net("f32x3")
    yield h
    h.close()


def _forward(net, frames, store=None):
    """-> (Q, workspace records, census, copied, the two destination buffers with their guard rows, or None)
    store = (first, first2, ring, second source)"""
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
    dst = dst2 = None
    copied = C.c_int(-1)
    with capi.launch_census() as census:
        if store is None:
            capi.check(capi.lib.rela_ffnet_forward(net.h, n, ptr(frames), ptr(legal), ptr(q), ptr(ws), nb, stream), "forward")
        else:
            first, first2, ring, src2 = store
            dst = torch.full(((ring + 2) * FRAME,), 0xA5, dtype=torch.uint8, device="cuda")
            dst2 = torch.full(((ring + 2) * FRAME,), 0xA5, dtype=torch.uint8, device="cuda")
            capi.check(capi.lib.rela_ffnet_debug_forward_store_frames2(
                net.h, n, ptr(frames), ptr(legal), ptr(q), ptr(ws), nb, C.c_void_p(dst.data_ptr() + FRAME), first, ring,
                ptr(src2), C.c_void_p(dst2.data_ptr() + FRAME), first2, C.byref(copied), stream), "forward_store_frames2")
        torch.cuda.synchronize()
    recs = ws[view.rec2:view.rec2 + n * (81 * 384 + 49 * 384)].cpu().numpy()  # (a2's records, then a3's)
    out = tuple(d.cpu().numpy().reshape(-1, FRAME) for d in (dst, dst2)) if dst is not None else None
    return q.cpu().numpy(), recs, dict(census.counts), copied.value, out


def _check_ring(rows_with_guards, first, n, ring, want, what):
    assert (rows_with_guards[0] == 0xA5).all() and (rows_with_guards[-1] == 0xA5).all(), what + ": guard row written"
    rows = rows_with_guards[1:-1]
    assert rows.shape[0] == ring
    slots = (first + np.arange(n)) % ring
    assert np.array_equal(rows[slots], want), what + ": rows are not the source frames"
    rest = np.setdiff1d(np.arange(ring), slots)
    assert rest.size == ring - n and (rows[rest] == 0xA5).all(), what + ": rows outside the block written"


@pytest.mark.parametrize("n", ROWS)
def test_copy2_keeps_the_bits_and_stores_both_sets_of_frames(net, n):
    import torch

    from synth import synth_obs

    host, host2 = synth_obs(n, 7000 + n), synth_obs(n, 9000 + n)
    assert not np.array_equal(host, host2)
    frames, frames2 = torch.from_numpy(host).cuda(), torch.from_numpy(host2).cuda()
    q0, rec0, ran0, _, _ = _forward(net, frames)
    assert ran0.get("conv12_s3") == 1 and "conv12_s3_copy" not in ran0 and "conv12_s3_copy2" not in ran0, ran0
    assert rec0 is not None and rec0.any()
    ring = n + EXTRA
    first, first2 = ring - 100, ring - 7  # both blocks wrap, at different rows
    q1, rec1, ran1, copied, (dst, dst2) = _forward(net, frames, (first, first2, ring, frames2))
    assert copied == 2
    assert ran1.get("conv12_s3_copy2") == 1 and ran1.get("conv12_s3") == 1 and "conv12_s3_copy" not in ran1, ran1
    assert np.array_equal(rec1, rec0), "workspace records differ from the ordinary forward's"
    assert np.array_equal(q1.view(np.uint32), q0.view(np.uint32))
    _check_ring(dst, first, n, ring, host.reshape(n, FRAME), "first destination")
    _check_ring(dst2, first2, n, ring, host2.reshape(n, FRAME), "second destination")


@pytest.mark.parametrize("precision,n", [("f32", 512), ("bf16x2", 512), ("f32x3", 128)])
def test_other_trunks_report_no_field_copied(precision, n):
    import torch

    from synth import synth_obs

    h = _net(precision)
    try:
        frames = torch.from_numpy(synth_obs(n, 7000)).cuda()
        frames2 = torch.from_numpy(synth_obs(n, 9000)).cuda()
        q0, _, ran0, _, _ = _forward(h, frames)
        q1, _, ran1, copied, (dst, dst2) = _forward(h, frames, (3, 5, n + EXTRA, frames2))
        assert copied == 0
        assert ran1 == ran0 and "conv12_s3_copy2" not in ran1 and "conv12_s3_copy" not in ran1, ran1
        assert (dst == 0xA5).all() and (dst2 == 0xA5).all()
        assert np.array_equal(q1.view(np.uint32), q0.view(np.uint32))
    finally:
        h.close()
