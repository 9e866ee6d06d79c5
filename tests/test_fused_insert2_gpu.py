"""The Ape-X shard's fused insert in mode 2 (csrc/actor.hip, rela_apex_actor_set_fused_insert(2)) stores the same replay.

In mode 2 (the default), where the target net's forward of post_step runs conv12_s3 (f32x3, 512 rows and up) and the
shard enters the replay as one block of plain rows, that forward writes next_obs into the block's rows from the
registers it stages the frames in AND passes obs, the frames acted on n ticks ago, through to the block's obs rows
(conv12_s3_copy2, rela_replay_direct_rows for both fields); the insert then copies eight small fields and launches no
replay_scatter_rows.  Nothing a reader of the replay can see may change, so the same seeded tick sequence runs in mode 2
and in mode 0 (every field copied by the insert), and after every insert the block's rows of all ten fields
(rela_replay_debug_read_rows, the ring's wrap followed), the priorities, the Q table of the tick's act(), the weights of
the whole ring and sum_ are compared with exact equality -- as are the ids, rows and IS weights of every sample.  In the
plain schema the stored obs / next_obs rows are also compared with the frames of n ticks ago / of this tick.

The run helper is the one of tests/test_fused_insert_gpu.py (copied: that file stays as it is) with the mode as a
number, the capacity as a parameter and an online weight reload: at tick N_STEP + 1 the online net gets new weights
between act() and post_step, so that tick's two online forwards -- and the obs forward of the next N_STEP ticks -- are
recomputed (the Q tables act() left are of another weight version) and read obs_t on the stream ahead of the forward
that passes it through.

Shapes: as there -- R = 512 and 513 are the smallest that reach conv12_s3, 513 makes blocks own one and two frames;
K = 64 and 57; n = 3; a ring of 5 R + 100 slots with capacity 4 / 5 of it, so the sixth insert starts ring - 100 slots
in, wraps, and rewrites the slots a sample has just evicted.  The decoupled insert form runs once at R = 512.

Census (note_launch) per insert in mode 2: no replay_scatter_rows, one conv12_s3_copy2, no conv12_s3_copy, and one
conv12_s3 launch (the target forward's; it is counted under both names) -- plus one per online forward the reload makes
post_step recompute: 3, 2, 2, 2 at the tick of the reload and the N_STEP after it, in either mode.  Every other case has the census of mode 0 and equal contents: f32 and bf16x2 nets (another trunk), R = 128
(below conv12_s3's 512 rows), dedup = "stack" and "plane" (reference rows; no replay_scatter_rows in any mode), and a
shard that goes in pieces (ring - capacity = 320 < R = 512: blocks of 320 and 192 rows, two replay_scatter_rows each).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, N_STEP = 18, 3
FRAME = 4 * 84 * 84
BATCH = 64
RELOAD_TICK = N_STEP + 1

_frames = {}


def frames_of(R, ticks):
    """[ticks][R][4][84][84] u8, seeded; made once per R and shared by the runs that compare against each other"""
    if R not in _frames or _frames[R].shape[0] < ticks:
        _frames[R] = np.random.default_rng(900 + R).integers(0, 256, (ticks, R, 4, 84, 84), dtype=np.uint8)
    return _frames[R]


def read_block(replay, field, first, count, ring):
    from rela_amd import _capi as capi

    rb = replay.row_bytes[field]
    if replay.dedup and field < 2:  # a de-duplicated stack field holds int32 references, one per unit of the stack
        rb = 4 * {"stack": 1, "plane": 4}[replay.dedup]
    out = np.zeros((count, rb), np.uint8)
    head = min(count, ring - first)
    for dst0, slot, cnt in ((0, first, head), (head, 0, count - head)):
        if cnt > 0:
            part = out[dst0:dst0 + cnt]
            capi.check(capi.lib.rela_replay_debug_read_rows(replay.h, field, slot, cnt, part.ctypes.data_as(C.c_void_p)),
                       "debug_read_rows")
    return out


def run(R, K, precision, mode, ticks, *, cap=None, dedup=None, decoupled=False, sample_after=()):
    """-> (trace, per-insert census, first slot of every inserted block, ring)"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.replay import FFReplay
    from synth import synth_params

    dev = "cuda:0"
    if cap is None:
        assert (5 * R + 100) % 5 == 0
        cap = (5 * R + 100) * 4 // 5
    on, tg = FFNetHandle(A, dev), FFNetHandle(A, dev)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 61).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 62).items()})
    on.set_precision(precision)
    tg.set_precision(precision)
    replay = FFReplay(cap, 7, 0.6, 0.4, 0, A, dev, dedup=dedup, guard_units=(N_STEP + 8) * R if dedup else 0)
    st = capi.ReplayState()
    capi.check(capi.lib.rela_replay_debug_state(replay.h, C.byref(st), None, None, None), "debug_state")
    ring = st.ring
    assert ring * 4 == cap * 5, (ring, cap)
    capi.check(capi.lib.rela_replay_set_decoupled_insert(replay.h, int(decoupled)), "set_decoupled_insert")
    eng = ApexActorEngine(R, K, A, N_STEP, 0.99, replay, [0.1] * R, dev, seed=5)
    eng.set_fused_insert(mode)
    frames = frames_of(R, ticks)
    rng = np.random.default_rng(77)
    trace, censuses, firsts = [], [], []
    inserts = 0
    for t in range(ticks):
        eng.next_obs_slot().copy_(torch.from_numpy(frames[t]))
        act = eng.act(on).cpu().numpy().copy()
        q = eng.q[0].cpu().numpy().copy()
        if t == RELOAD_TICK:  # new online weights between act() and post_step: the cached Q tables are stale
            on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 63).items()})
        rew = torch.from_numpy(rng.integers(-1, 2, R).astype(np.float32)).to(dev)
        term = torch.from_numpy((rng.uniform(size=R) < 0.1).astype(np.uint8)).to(dev)
        first = replay.debug_state()["tail"]
        with capi.launch_census() as census:
            inserted = eng.post_step(rew, term, on, tg, nonblocking=True)
        assert inserted == (t >= N_STEP), (t, capi.lib.rela_last_error())
        if not inserted:
            continue
        inserts += 1
        torch.cuda.synchronize()
        censuses.append(dict(census.counts))
        firsts.append(first)
        rows = [read_block(replay, f, first, R, ring) for f in range(10)]
        if dedup is None:  # the frames themselves: obs of n ticks ago, next_obs of this tick
            assert np.array_equal(rows[0], frames[t - N_STEP].reshape(R, FRAME)), (t, "obs rows")
            assert np.array_equal(rows[1], frames[t].reshape(R, FRAME)), (t, "next_obs rows")
        w = np.zeros(ring, np.float32)
        capi.check(capi.lib.rela_replay_debug_weights(replay.h, w.ctypes.data_as(C.c_void_p), None), "debug_weights")
        state = replay.debug_state()
        trace.append(("insert", t, first, [r.tobytes() for r in rows], eng.prio.cpu().numpy().tobytes(), q.tobytes(),
                      act.tobytes(), w.tobytes(), state["sum"], state["size"], state["head"], state["tail"]))
        if inserts in sample_after:
            batch, weight = replay.sample(BATCH)
            torch.cuda.synchronize()
            ids = np.zeros(BATCH, np.int32)
            capi.check(capi.lib.rela_replay_debug_state(replay.h, C.byref(st), ids.ctypes.data_as(C.c_void_p), None, None),
                       "debug_state")
            trace.append(("sample", ids.tobytes(), batch.obs["s"].cpu().numpy().tobytes(),
                          batch.next_obs["s"].cpu().numpy().tobytes(), batch.action["a"].cpu().numpy().tobytes(),
                          batch.reward.cpu().numpy().tobytes(), weight.cpu().numpy().tobytes(), st.head, st.size))
            replay.update_priority(torch.from_numpy(rng.uniform(0.05, 3.0, BATCH).astype(np.float32)))
    torch.cuda.synchronize()
    eng.close()
    replay.close()
    on.close()
    tg.close()
    return trace, censuses, firsts, ring


def assert_same(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x[:3] == y[:3] or x[0] == "sample"
        assert len(x) == len(y)
        for i, (u, v) in enumerate(zip(x, y)):
            assert u == v, (x[0], x[1] if x[0] == "insert" else None, "item %d differs" % i)


@pytest.mark.parametrize("R,K,decoupled", [(512, 64, False), (513, 57, False), (512, 64, True)])
def test_mode_2_stores_the_same_replay_without_row_copies(R, K, decoupled):
    ticks = N_STEP + 7
    kw = dict(decoupled=decoupled, sample_after=(5, 6))
    t2, c2, firsts, ring = run(R, K, "f32x3", 2, ticks, **kw)
    t0, c0, firsts0, _ = run(R, K, "f32x3", 0, ticks, **kw)
    assert firsts == firsts0
    # the sixth block starts ring - 100 slots in, wraps, and lands on slots the sample before it evicted
    assert firsts[5] == ring - 100 and firsts[5] + R > ring, firsts
    # conv12_s3 launches of an insert: the target forward alone, plus the online forwards post_step recomputes -- both at
    # the tick of the reload, the one of obs at the N_STEP ticks after it (act() saw those frames with the old weights)
    forwards = [1 + (2 if t == RELOAD_TICK else 1 if RELOAD_TICK < t <= RELOAD_TICK + N_STEP else 0) for t in range(N_STEP, ticks)]
    assert forwards == [1, 3, 2, 2, 2, 1, 1]
    assert len(c2) == len(c0) == len(forwards)
    for c, want in zip(c2, forwards):
        assert "replay_scatter_rows" not in c and c.get("conv12_s3_copy2") == 1 and "conv12_s3_copy" not in c, c
        assert c.get("conv12_s3") == want, c
    for c, want in zip(c0, forwards):
        assert c.get("replay_scatter_rows") == 2 and "conv12_s3_copy" not in c and "conv12_s3_copy2" not in c, c
        assert c.get("conv12_s3") == want, c
    assert_same(t2, t0)


@pytest.mark.parametrize("R,K,precision,dedup,cap", [(512, 64, "f32", None, None), (512, 64, "bf16x2", None, None),
                                                     (512, 64, "f32x3", "stack", None), (512, 64, "f32x3", "plane", None),
                                                     (128, 64, "f32x3", None, None), (512, 64, "f32x3", None, 1280)])
def test_other_cases_take_the_unfused_path(R, K, precision, dedup, cap):
    ticks = N_STEP + 2
    t2, c2, _, _ = run(R, K, precision, 2, ticks, cap=cap, dedup=dedup, sample_after=(2,))
    t0, c0, _, _ = run(R, K, precision, 0, ticks, cap=cap, dedup=dedup, sample_after=(2,))
    assert c2 == c0
    pieces = 2 if cap else 1
    for c in c2:
        assert "conv12_s3_copy" not in c and "conv12_s3_copy2" not in c, c
        assert c.get("replay_scatter_rows", 0) == (0 if dedup else 2 * pieces), c  # (dedup: small reference rows)
    assert_same(t2, t0)
