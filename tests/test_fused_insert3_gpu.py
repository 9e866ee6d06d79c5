"""The Ape-X shard's fused insert in mode 3 (csrc/actor.hip, rela_apex_actor_set_fused_insert(3), the default) stores the
same replay.

In mode 3, where mode 2 applies and the target forward stored both frame fields, the TD kernel of post_step finishes the
block (csrc/agent_ops.hip: td_kernel_insert): besides the priorities it stores the row's eight small fields (eps x2,
legal_move x2, action, reward, terminal, bootstrap) into the block's replay rows and the row's weight pow(priority, alpha)
into the replay's weight ring (rela_replay_direct_small), and the commit is replay_append_sums alone
(rela_replay_commit_add_weighted).  Nothing a reader of the replay can see may change, so the same seeded tick sequence
runs in mode 3 and in mode 2, and after every insert the block's rows of all ten fields (the ring's wrap followed), the
actor's priorities, the weights of the whole ring (d_w) and sum_ / size / head / tail are compared with torch.equal / ==,
as are the ids and IS weights of every sample -- one after the fifth insert, which evicts, and sample(64) at the end.

Shapes: R = 512 is the smallest shard that takes conv12_s3; 513 = 9 x 57 and 769 = 1 x 769 are multiples neither of a
tile nor of the 256 threads of a workgroup, K = 769 is one reference block of more than 512 rows (a 1,024-thread
workgroup that strides), and at K = 64 / 57 the pow routine's tail (the last K mod 32 rows of every block take the scalar
double pow) covers 0 and 25 rows; R = 1083 = 19 x 57 is past the 1,024 rows from which mode 2 commits with
replay_append_pow + replay_append_sums instead of the one-workgroup replay_append_weights.  n = 3, alpha = 0.6, a ring of
5 R + 100 slots with capacity 4 / 5 of it: the sixth insert starts ring - 100 slots in, wraps (first_slot + R > ring), and
rewrites slots the sample before it evicted.

Census (note_launch) of every mode-3 insert: one td_kernel_insert, one replay_append_sums, one conv12_s3_copy2, and no
replay_scatter_rows, replay_scatter_small, replay_append_pow or replay_append_weights; of every mode-2 insert: one
replay_scatter_small and the append of its size.

Fall-backs: with de-duplication on, with f32 nets (another trunk) and with the replay in its decoupled insert form, the
census and the contents of mode 3 equal mode 0's in every tick; with a ring that fills up (no sample, nonblocking) the
inserts that no longer fit are dropped with mode 0's census, and the ring ends with mode 0's contents.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, N_STEP = 18, 3
FRAME = 4 * 84 * 84
BATCH = 64
MAX_R, MAX_TICKS = 1083, N_STEP + 6

_frames = []


def frames_of(R, ticks):
    """[ticks][R][4][84][84] u8, seeded; made once and shared (as slices) by every run"""
    if not _frames:
        _frames.append(np.random.default_rng(903).integers(0, 256, (MAX_TICKS, MAX_R, 4, 84, 84), dtype=np.uint8))
    assert R <= MAX_R and ticks <= MAX_TICKS
    return _frames[0][:ticks, :R]


def read_rows(replay, field, first, count, ring):
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


def run(R, K, precision, mode, ticks, *, dedup=None, decoupled=False, sample_after=(), final_sample=False):
    """-> (records, ring); a record is (kind, tick, census, {name: array or number})"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.replay import FFReplay
    from synth import synth_params

    dev = "cuda:0"
    assert (5 * R + 100) % 5 == 0
    cap = (5 * R + 100) * 4 // 5
    on, tg = FFNetHandle(A, dev), FFNetHandle(A, dev)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 61).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 62).items()})
    on.set_precision(precision)
    tg.set_precision(precision)
    replay = FFReplay(cap, 7, 0.6, 0.4, 0, A, dev, dedup=dedup, guard_units=(N_STEP + 8) * R if dedup else 0)
    ring = replay.debug_state()["ring"]
    assert ring == 5 * R + 100
    capi.check(capi.lib.rela_replay_set_decoupled_insert(replay.h, int(decoupled)), "set_decoupled_insert")
    eng = ApexActorEngine(R, K, A, N_STEP, 0.99, replay, np.linspace(0.0, 0.4, R).tolist(), dev, seed=5)
    if mode is not None:  # None: the shard's default
        eng.set_fused_insert(mode)
    frames = frames_of(R, ticks)
    rng = np.random.default_rng(77)
    st = capi.ReplayState()

    def weights():
        w = np.zeros(ring, np.float32)
        capi.check(capi.lib.rela_replay_debug_weights(replay.h, w.ctypes.data_as(C.c_void_p), None), "debug_weights")
        return w

    def sample():
        batch, weight = replay.sample(BATCH)
        torch.cuda.synchronize()
        ids = np.zeros(BATCH, np.int32)
        capi.check(capi.lib.rela_replay_debug_state(replay.h, C.byref(st), ids.ctypes.data_as(C.c_void_p), None, None),
                   "debug_state")
        rec = ("sample", -1, {}, {"ids": ids, "is_weights": weight.cpu().numpy(), "obs": batch.obs["s"].cpu().numpy(),
                                  "next_obs": batch.next_obs["s"].cpu().numpy(), "action": batch.action["a"].cpu().numpy(),
                                  "reward": batch.reward.cpu().numpy(), "head": st.head, "size": st.size})
        replay.update_priority(torch.from_numpy(rng.uniform(0.05, 3.0, BATCH).astype(np.float32)))
        return rec

    records = []
    inserts = 0
    for t in range(ticks):
        eng.next_obs_slot().copy_(torch.from_numpy(np.ascontiguousarray(frames[t])))
        eng.legal.copy_(torch.from_numpy((rng.uniform(size=(R, A)) < 0.8).astype(np.float32)))
        eng.legal[:, 0] = 1.0
        eng.act(on)
        rew = torch.from_numpy(rng.integers(-1, 2, R).astype(np.float32)).to(dev)
        term = torch.from_numpy((rng.uniform(size=R) < 0.1).astype(np.uint8)).to(dev)
        first = replay.debug_state()["tail"]
        with capi.launch_census() as census:
            inserted = eng.post_step(rew, term, on, tg, nonblocking=True)
        torch.cuda.synchronize()
        if t < N_STEP:
            assert not inserted
            continue
        state = replay.debug_state()
        items = {"prio": eng.prio.cpu().numpy(), "d_w": weights(), "sum": state["sum"], "size": state["size"],
                 "head": state["head"], "tail": state["tail"]}
        if inserted:
            inserts += 1
            items["first"] = first
            for f in range(10):
                items["field%d" % f] = read_rows(replay, f, first, R, ring)
            if dedup is None:  # the frames themselves: obs of n ticks ago, next_obs of this tick
                assert np.array_equal(items["field0"], frames[t - N_STEP].reshape(R, FRAME)), (t, "obs rows")
                assert np.array_equal(items["field1"], frames[t].reshape(R, FRAME)), (t, "next_obs rows")
        records.append(("insert" if inserted else "drop", t, dict(census.counts), items))
        if inserted and inserts in sample_after:
            records.append(sample())
    if final_sample:
        records.append(sample())
    items = {"d_w": weights()}
    for f in range(10):
        items["field%d" % f] = read_rows(replay, f, 0, ring, ring)
    records.append(("end", ticks, {}, items))
    torch.cuda.synchronize()
    eng.close()
    replay.close()
    on.close()
    tg.close()
    return records, ring


def assert_same_contents(a, b):
    import torch

    assert [r[:2] for r in a] == [r[:2] for r in b] and len(a) > 0
    for (kind, t, _, x), (_, _, _, y) in zip(a, b):
        assert sorted(x) == sorted(y)
        for name in x:
            if isinstance(x[name], np.ndarray):
                assert x[name].dtype == y[name].dtype
                same = torch.equal(torch.from_numpy(x[name]), torch.from_numpy(y[name]))
            else:
                same = x[name] == y[name]
            assert same, (kind, t, name)


REPLAY_KERNELS = ("replay_scatter_rows", "replay_scatter_small", "replay_append_pow", "replay_append_sums",
                  "replay_append_weights", "td_kernel_insert", "conv12_s3_copy2", "conv12_s3_copy")


def insert_census(records):
    return [{k: c.get(k, 0) for k in REPLAY_KERNELS} for kind, _, c, _ in records if kind == "insert"]


@pytest.mark.parametrize("R,K", [(512, 64), (513, 57), (769, 769), (1083, 57)])
def test_mode_3_stores_the_same_replay_from_the_td_kernel(R, K):
    kw = dict(sample_after=(5,), final_sample=True)
    r3, ring = run(R, K, "f32x3", 3, N_STEP + 6, **kw)
    r2, _ = run(R, K, "f32x3", 2, N_STEP + 6, **kw)
    firsts = [x["first"] for kind, _, _, x in r3 if kind == "insert"]
    assert len(firsts) == 6
    # the sixth block starts ring - 100 slots in, wraps, and lands on slots the sample before it evicted
    assert firsts[5] == ring - 100 and firsts[5] + R > ring, firsts
    for c in insert_census(r3):
        assert c == {"replay_scatter_rows": 0, "replay_scatter_small": 0, "replay_append_pow": 0, "replay_append_sums": 1,
                     "replay_append_weights": 0, "td_kernel_insert": 1, "conv12_s3_copy2": 1, "conv12_s3_copy": 0}, c
    two_launch = R >= 1024  # (replay.hip, launch_append)
    for c in insert_census(r2):
        assert c == {"replay_scatter_rows": 0, "replay_scatter_small": 1, "replay_append_pow": int(two_launch),
                     "replay_append_sums": int(two_launch), "replay_append_weights": int(not two_launch),
                     "td_kernel_insert": 0, "conv12_s3_copy2": 1, "conv12_s3_copy": 0}, c
    assert_same_contents(r3, r2)


def test_mode_3_is_the_default():
    r, _ = run(512, 64, "f32x3", None, N_STEP + 1)
    assert [c["td_kernel_insert"] for c in insert_census(r)] == [1]


@pytest.mark.parametrize("precision,dedup,decoupled", [("f32", None, False), ("f32x3", "plane", False), ("f32x3", None, True)])
def test_other_cases_take_the_unfused_tail(precision, dedup, decoupled):
    kw = dict(dedup=dedup, decoupled=decoupled, sample_after=(2,))
    r3, _ = run(512, 64, precision, 3, N_STEP + 3, **kw)
    r0, _ = run(512, 64, precision, 0, N_STEP + 3, **kw)
    c3, c0 = insert_census(r3), insert_census(r0)
    assert len(c3) == 3
    for c in c3:
        assert c["td_kernel_insert"] == 0 and c["replay_scatter_small"] == 1 and c["replay_append_weights"] == 1, c
    if decoupled:  # the frames still go in from the forward (mode 2's part); the tail is the ordinary one
        for c, d in zip(c3, c0):
            assert c["conv12_s3_copy2"] == 1 and c["replay_scatter_rows"] == 0 and d["replay_scatter_rows"] == 2, (c, d)
            assert {k: c[k] for k in REPLAY_KERNELS[1:6]} == {k: d[k] for k in REPLAY_KERNELS[1:6]}, (c, d)
    else:
        assert [r[2] for r in r3] == [r[2] for r in r0]
    assert_same_contents(r3, r0)


@pytest.mark.parametrize("mode", [3, 2])
def test_the_eviction_list_stays_bounded(mode):
    """Every sample of a ring at capacity evicts and leaves an entry (slots, event) that the next writer of rows must wait
    for and that is retired once its gathers have finished.  A mode-3 tick never goes through write_rows, so the calls it
    does make (rela_replay_direct_rows / _direct_small) have to retire entries themselves: otherwise the list, the events
    created and the waits per tick grow with the length of the run.  24 rounds of tick + evicting sample, the sample
    synchronised before the next tick: then at most ONE eviction is outstanding at any time, so after a sample the list
    holds 1 entry, after a tick 0, the last writer of the tick was given 0 waits, and list + pool never hold more than the
    one event that goes round (rela_replay_debug_evictions)."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.replay import FFReplay
    from synth import synth_params

    dev, R, K, rounds = "cuda:0", 512, 64, 24
    on, tg = FFNetHandle(A, dev), FFNetHandle(A, dev)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 61).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 62).items()})
    on.set_precision("f32x3")
    tg.set_precision("f32x3")
    replay = FFReplay((5 * R + 100) * 4 // 5, 7, 0.6, 0.4, 0, A, dev)
    eng = ApexActorEngine(R, K, A, N_STEP, 0.99, replay, [0.1] * R, dev, seed=5)
    eng.set_fused_insert(mode)
    frames = frames_of(R, MAX_TICKS)
    rew = torch.zeros(R, device=dev)
    term = torch.zeros(R, dtype=torch.uint8, device=dev)

    def evictions():
        v = [C.c_int(-1), C.c_int(-1), C.c_int(-1)]
        capi.check(capi.lib.rela_replay_debug_evictions(replay.h, *[C.byref(x) for x in v]), "debug_evictions")
        return tuple(x.value for x in v)  # (pending, pooled, last_waits)

    inserts = 0
    for t in range(N_STEP + 5 + rounds):
        eng.next_obs_slot().copy_(torch.from_numpy(np.ascontiguousarray(frames[t % MAX_TICKS])))
        eng.act(on)
        with capi.launch_census() as census:
            inserted = eng.post_step(rew, term, on, tg, nonblocking=True)
        assert inserted == (t >= N_STEP), t
        if not inserted:
            continue
        inserts += 1
        assert census.counts.get("td_kernel_insert", 0) == int(mode == 3), census.counts
        pending, pooled, waits = evictions()
        assert pending == 0 and waits == 0 and pooled <= 1, (t, pending, pooled, waits)
        if inserts >= 5:  # the ring is over capacity: this sample evicts
            head = replay.debug_state()["head"]
            replay.sample(BATCH)
            torch.cuda.synchronize()
            assert replay.debug_state()["head"] != head, t
            pending, pooled, _ = evictions()
            assert pending == 1 and pooled == 0, (t, pending, pooled)
            replay.update_priority(torch.full((BATCH,), 0.5))
    assert inserts == 5 + rounds
    torch.cuda.synchronize()
    eng.close()
    replay.close()
    on.close()
    tg.close()


def test_a_full_ring_drops_the_insert_as_before():
    r3, _ = run(512, 64, "f32x3", 3, N_STEP + 6)  # no sample: five blocks fit, the sixth does not
    r0, _ = run(512, 64, "f32x3", 0, N_STEP + 6)
    assert [r[0] for r in r3] == ["insert"] * 5 + ["drop", "end"]
    drops3 = [r[2] for r in r3 if r[0] == "drop"]
    assert drops3 == [r[2] for r in r0 if r[0] == "drop"]
    assert not any(k in drops3[0] for k in REPLAY_KERNELS), drops3
    assert_same_contents(r3, r0)
