"""Frame-stack de-duplication in the SEQUENCE replay (RNNPrioritizedReplay, rela/types.h:53-73): the T stacks of an R2D2
sequence are kept as [T][1 or 4] references into the replay's unit ring (csrc/replay.hip:
rela_replay_set_schema_seq_dedup; csrc/actor_r2d2.hip: rela_r2d2_actor_set_dedup).  Parity definition as in
tests/test_dedup_gpu.py: every sampled batch is IDENTICAL to the batch of a replay that stores the stacks in full, fed
by the same actor shard inputs."""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE = 84 * 84
FIELDS = ("s", "eps", "legal_move", "a", "reward", "terminal", "bootstrap", "h0", "c0", "seq_len")


class _Planes:
    """planes[t] ([R][84][84], made on demand): the env's stack at tick t is its last four planes, restarted after a
    terminal with the first plane repeated four times (atari/game_state.h:53-82).  Plane bytes (0, 0) / (0, 1) carry the
    tags tick % 251 / row % 251."""

    def __init__(self, seed, R):
        self.seed, self.R, self.cache = seed, R, {}

    def __getitem__(self, key):
        t, rest = (key[0], key[1:]) if isinstance(key, tuple) else (key, ())
        if t not in self.cache:
            p = np.random.default_rng((self.seed, t)).integers(1, 256, (self.R, 84, 84), dtype=np.uint8)
            p[:, 0, 0] = t % 251
            p[:, 0, 1] = (np.arange(self.R) % 251).astype(np.uint8)
            if len(self.cache) > 64:
                self.cache.pop(next(iter(self.cache)))
            self.cache[t] = p
        return self.cache[t][rest] if rest else self.cache[t]


def _sliding_stream(rng, R, ticks, p_term):
    """(planes, terminals [ticks][R])"""
    planes = _Planes(int(rng.integers(1 << 30)), R)
    term = (rng.uniform(size=(ticks, R)) < p_term).astype(np.uint8)
    return planes, term


def _stacks_at(planes, term, t, prev):
    """the [R,4,84,84] stacks of tick t given those of tick t - 1 (None at t = 0)"""
    R = planes.R
    out = np.empty((R, 4, 84, 84), np.uint8)
    for r in range(R):
        if prev is None or term[t - 1, r]:
            out[r, :] = planes[t, r]
        else:
            out[r, :3] = prev[r, 1:]
            out[r, 3] = planes[t, r]
    return out


def _lstm(A, seed, dev, precision):
    import torch

    from rela_amd.engine import LSTMNetHandle
    from synth import synth_lstm_params

    h = LSTMNetHandle(A, dev)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, seed).items()})
    if precision != "f32":
        h.set_precision(precision)
    return h


def _engines(modes, R, K, A, n, seq, burn, cap, dev, guard, units_per_slot=None):
    from rela_amd.engine import R2D2ActorEngine
    from rela_amd.replay import RNNReplay

    T = burn + seq + n
    out = []
    for mode in modes:
        rp = RNNReplay(cap, 7, 0.6, 0.4, 0, A, T, dev, dedup=mode, guard_units=guard,
                       units_per_slot=units_per_slot or seq + n)
        out.append((rp, R2D2ActorEngine(R, K, A, n, 0.997, seq, burn, 0.9, rp, [0.0] * R, dev)))
    return out


@pytest.mark.parametrize("shape", ["small", "c4"])
@pytest.mark.parametrize("mode", ["stack", "plane"])
def test_seq_dedup_batches_identical_to_full_storage(mode, shape):
    """A full-storage and a de-duplicated RNNReplay, each fed by its own R2D2 shard with the same inputs, sampled in lock
    step: ids, all ten fields, IS weights, head / size and the f64 sum must agree exactly.  Random terminals (some in the
    carried region: second, short sequences; front and tail padding), until the slot ring and the unit ring wrapped."""
    import torch

    from rela_amd import _capi as capi

    if shape == "small":
        R, K, n, seq, burn, cap, ticks, p_term, batch = 16, 4, 3, 8, 4, 128, 260, 0.06, 16
    else:  # BASELINE C4's sequence shape
        R, K, n, seq, burn, cap, ticks, p_term, batch = 256, 64, 3, 80, 40, 2048, 1150, 0.004, 32
    T = burn + seq + n
    A, dev = 6, "cuda:0"
    rng = np.random.default_rng(41 if mode == "stack" else 42)
    planes, term = _sliding_stream(rng, R, ticks, p_term)
    rewards = rng.integers(-1, 2, (ticks, R)).astype(np.float32)
    on, tg = _lstm(A, 1, dev, "f32"), _lstm(A, 2, dev, "f32")
    guard = (2 * T + n + 10) * R
    (rf, ef), (rd, ed) = _engines([None, mode], R, K, A, n, seq, burn, cap, dev, guard)
    ucap = C.c_int64()
    capi.check(capi.lib.rela_replay_dedup_info(rd.h, None, None, C.byref(ucap)), "dedup_info")
    units_per_tick = R
    prev = None
    nsamp, heads = 0, set()
    ids_f, ids_d = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
    for t in range(ticks):
        stacks = _stacks_at(planes, term, t, prev)
        prev = stacks
        src = torch.from_numpy(stacks).to(dev)
        for rp, eng in ((rf, ef), (rd, ed)):
            eng.next_obs_slot().copy_(src)
            eng.act(on)
            eng.post_step(rewards[t], term[t], on, tg)
        if rf.size() >= batch:
            assert rd.size() == rf.size()
            bf, wf = rf.sample(batch, slot=0)
            bd, wd = rd.sample(batch, slot=0)
            torch.cuda.synchronize()
            sf, sd = capi.ReplayState(), capi.ReplayState()
            capi.check(capi.lib.rela_replay_debug_state(rf.h, C.byref(sf), ids_f.ctypes.data_as(C.c_void_p), None, None), "st")
            capi.check(capi.lib.rela_replay_debug_state(rd.h, C.byref(sd), ids_d.ctypes.data_as(C.c_void_p), None, None), "st")
            assert sd.dev_error == 0 and sf.dev_error == 0
            assert np.array_equal(ids_f, ids_d), t
            outf, outd = rf._buffers(batch, 0), rd._buffers(batch, 0)
            for f in FIELDS + ("weight",):
                assert torch.equal(outf[f], outd[f]), (mode, shape, t, f)
            assert (sf.sum, sf.head, sf.size, sf.num_add) == (sd.sum, sd.head, sd.size, sd.num_add), t
            heads.add(sf.head)
            nsamp += 1
            p = torch.linspace(0.3, 1.7, batch, device=dev) * (1 + (t % 5) * 0.1)
            rf.update_priority(p)
            rd.update_priority(p)
    st = rd.debug_state()
    ring = int(1.25 * cap)
    assert st["num_add"] > ring and nsamp > 20  # the slot ring wrapped
    assert ticks * units_per_tick > ucap.value  # ... and the unit ring
    for rp, eng in ((rf, ef), (rd, ed)):
        eng.close()
        rp.close()


def _hand_replay(ups, T, nslots, units, refs, A=4):
    """An RNNReplay-shaped partition filled through the ABI: `units` [U][unit bytes] go into the unit ring, slot i
    gets the references refs[i] ([T][ups]), all other fields zero."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.replay import RNNReplay

    dev = "cuda:0"
    U = units.shape[0]
    rp = RNNReplay(nslots, 3, 1.0, 1.0, 0, A, T, dev, dedup={1: "stack", 4: "plane"}[ups], guard_units=U, units_per_slot=1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    first, idx = C.c_int64(), C.c_int32()
    capi.check(capi.lib.rela_replay_units_reserve(rp.h, U, 0, C.byref(first), C.byref(idx)), "reserve")
    assert first.value == 0 and idx.value == 0
    u_dev = torch.from_numpy(units).to(dev)
    capi.check(capi.lib.rela_replay_units_write(rp.h, 0, U, C.c_void_p(u_dev.data_ptr()), units.shape[1], stream), "write")
    rb = [T * 4 * ups, T * 4, T * 4 * A, T * 8, T * 4, T, T * 4, 2048, 2048, 4]
    keep = [torch.from_numpy(np.ascontiguousarray(refs, np.int32)).to(dev)]
    keep += [torch.zeros(nslots * b, dtype=torch.uint8, device=dev) for b in rb[1:]]
    slot = C.c_int()
    capi.check(capi.lib.rela_replay_begin_add(rp.h, nslots, 0, C.byref(slot)), "begin_add")
    capi.check(capi.lib.rela_replay_set_block_min_unit(rp.h, slot.value, nslots, 0), "min_unit")
    rows = (C.c_void_p * 10)(*[k.data_ptr() for k in keep])
    capi.check(capi.lib.rela_replay_write_rows(rp.h, slot.value, 0, nslots, rows, stream), "write_rows")
    prio = torch.linspace(0.5, 1.5, nslots, device=dev)
    capi.check(capi.lib.rela_replay_commit_add(rp.h, slot.value, nslots, C.c_void_p(prio.data_ptr()), stream), "commit")
    torch.cuda.synchronize()
    return rp, keep


def test_seq_dedup_gather_layout():
    """The sequence gather against a numpy restatement: -1 padding (front and tail), a keyframe, an episode start (first
    plane repeated four times), sliding stacks, and B * T * 4 = 78,720 output planes (> 65,535 grid rows)."""
    import torch

    from rela_amd import _capi as capi

    rng = np.random.default_rng(9)
    T, nslots, B, U = 123, 6, 160, 700
    units = rng.integers(0, 256, (U, PLANE), dtype=np.uint8)
    refs = np.full((nslots, T, 4), -1, np.int64)
    for i in range(nslots):
        base = rng.integers(0, U - 4 * T)
        t0 = int(rng.integers(0, 20))  # front padding
        t1 = T - int(rng.integers(0, 20))  # tail padding
        cur = [base, base + 1, base + 2, base + 3]  # keyframe
        nxt = base + 4
        for t in range(t0, t1):
            if t > t0:
                if t == t0 + 30 + i:  # an episode start: the new plane four times
                    cur = [nxt] * 4
                else:
                    cur = cur[1:] + [nxt]
                nxt += 1
            refs[i, t] = cur
    refs %= U
    refs[refs < 0] = -1
    refs = np.where(refs < 0, -1, refs)
    rp, keep = _hand_replay(4, T, nslots, units, refs.astype(np.int32))
    b, w = rp.sample(B)
    torch.cuda.synchronize()
    ids = np.zeros(B, np.int32)
    st = capi.ReplayState()
    capi.check(capi.lib.rela_replay_debug_state(rp.h, C.byref(st), ids.ctypes.data_as(C.c_void_p), None, None), "st")
    got = b.obs["s"].cpu().numpy()  # [T, B, 4, 84, 84]
    zero_or = np.concatenate([units, np.zeros((1, PLANE), np.uint8)])  # index -1 -> the zero plane
    want = zero_or[refs[ids]].reshape(B, T, 4, 84, 84).transpose(1, 0, 2, 3, 4)
    assert np.array_equal(got, want)
    assert len(set(ids.tolist())) > 1
    rp.close()


def test_seq_dedup_stack_units_gather_layout():
    """units_per_stack = 1: a reference per stack, -1 = a zero stack."""
    import torch

    from rela_amd import _capi as capi

    rng = np.random.default_rng(10)
    T, nslots, B, U = 15, 5, 64, 60
    units = rng.integers(0, 256, (U, 4 * PLANE), dtype=np.uint8)
    refs = rng.integers(-1, U, (nslots, T, 1)).astype(np.int32)
    rp, keep = _hand_replay(1, T, nslots, units, refs)
    b, w = rp.sample(B)
    torch.cuda.synchronize()
    ids = np.zeros(B, np.int32)
    st = capi.ReplayState()
    capi.check(capi.lib.rela_replay_debug_state(rp.h, C.byref(st), ids.ctypes.data_as(C.c_void_p), None, None), "st")
    zero_or = np.concatenate([units, np.zeros((1, 4 * PLANE), np.uint8)])
    want = zero_or[refs[ids, :, 0]].reshape(B, T, 4, 84, 84).transpose(1, 0, 2, 3, 4)
    assert np.array_equal(b.obs["s"].cpu().numpy(), want)
    rp.close()


def _check_sequences_by_tags(s, planes, term_rows=None):
    """s: [T, B, 4, 84, 84] numpy.  Every stack is all zero (padding) or the true stack of its env at its tick (read off
    the newest plane's tags); the real stacks of one sequence are consecutive ticks of one env."""
    T, B = s.shape[:2]
    checked = 0
    for b in range(B):
        last = None
        for t in range(T):
            st = s[t, b]
            if not st.any():
                continue
            tick, row = int(st[3, 0, 0]), int(st[3, 0, 1])
            assert np.array_equal(st[3], planes[tick, row]), (b, t)
            for k in range(3):  # older planes: the env's earlier ticks, clamped at the episode's (here: run's) start
                assert np.array_equal(st[k], planes[max(tick - 3 + k, 0), row]), (b, t, k)
            if last is not None:
                assert (tick, row) == (last[0] + 1, last[1]), (b, t)
            last = (tick, row)
            checked += 1
    return checked


def test_seq_dedup_survives_dropped_blocks():
    """A tiny ring with nonblocking inserts: pieces are dropped, and ticks whose planes do not fit are not stored (the
    shard drops every sequence containing one, and restarts the planes with a keyframe).  Whatever is sampled must be
    the env's true stacks."""
    import torch

    R, K, n, seq, burn, cap, ticks, batch = 8, 4, 2, 6, 3, 16, 200, 8
    T = burn + seq + n
    A, dev = 5, "cuda:0"
    rng = np.random.default_rng(6)
    planes, term = _sliding_stream(rng, R, ticks, 0.0)  # one episode per env: the tags stay unambiguous
    on, tg = _lstm(A, 1, dev, "f32"), _lstm(A, 2, dev, "f32")
    (rp, eng), = _engines(["plane"], R, K, A, n, seq, burn, cap, dev, guard=(2 * T + n + 10) * R)
    prev, nsamp, checked, dropped = None, 0, 0, 0
    for t in range(ticks):
        stacks = _stacks_at(planes, term, t, prev)
        prev = stacks
        eng.next_obs_slot().copy_(torch.from_numpy(stacks).to(dev))
        eng.act(on)
        before = rp.num_add()
        eng.post_step(np.zeros(R, np.float32), term[t], on, tg, nonblocking=True)
        if t % 9 == 8 and rp.size() >= batch:
            b, w = rp.sample(batch)
            st = rp.debug_state()
            assert st["dev_error"] == 0
            checked += _check_sequences_by_tags(b.obs["s"].cpu().numpy(), planes)
            rp.update_priority(torch.ones(batch, device=dev))
            nsamp += 1
    assert nsamp >= 10 and checked > 0
    assert rp.num_add() < (ticks // seq) * R  # sequences were dropped
    eng.close()
    rp.close()


def test_seq_dedup_unit_budget_exceeded_hands_out_no_wrong_frames():
    """A unit ring far below the budget (one unit per slot, no guard: less than one window's reach) must not hand out
    wrong frames: ticks that do not fit are not stored (their sequences dropped), or the shard stops loudly with
    RELA_ESTATE from rela_replay_set_block_min_unit."""
    import torch

    from rela_amd import _capi as capi

    R, K, n, seq, burn, cap, ticks, batch = 4, 4, 2, 6, 3, 64, 80, 4
    A, dev = 5, "cuda:0"
    planes, term = _sliding_stream(np.random.default_rng(8), R, ticks, 0.0)
    on, tg = _lstm(A, 1, dev, "f32"), _lstm(A, 2, dev, "f32")
    (rp, eng), = _engines(["plane"], R, K, A, n, seq, burn, cap, dev, guard=0, units_per_slot=1)
    prev, err, checked = None, None, 0
    for t in range(ticks):
        stacks = _stacks_at(planes, term, t, prev)
        prev = stacks
        eng.next_obs_slot().copy_(torch.from_numpy(stacks).to(dev))
        eng.act(on)
        try:
            eng.post_step(np.zeros(R, np.float32), term[t], on, tg, nonblocking=True)
        except RuntimeError as e:
            err = e
            break
        if rp.size() >= batch:
            b, w = rp.sample(batch)
            checked += _check_sequences_by_tags(b.obs["s"].cpu().numpy(), planes)
            rp.update_priority(torch.ones(batch, device=dev))
    assert err is None or (err.code == capi.ESTATE and "overwritten" in str(err)), err
    assert err is not None or rp.num_add() < (ticks // seq) * R  # the budget was exceeded: something gave way
    eng.close()
    rp.close()


def test_seq_dedup_reference_capacity_on_one_gpu():
    """run_r2d2.sh's replay (capacity 65,536: 81,920 slots of 123 stacks, 284 GB in full) in plane units on one GPU,
    fed by 3,200 envs at C4's sequence shape until the slot ring and the unit ring wrapped; sampled sequences are
    checked IN FULL on the device against the tags of their planes.  The replay's allocation must stay under 60 GB."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import R2D2ActorEngine
    from rela_amd.replay import RNNReplay

    free0, _ = torch.cuda.mem_get_info()
    if free0 < 90e9:
        pytest.skip("needs ~90 GB of free HBM")
    R, K, n, seq, burn, A, dev = 3200, 3200, 3, 80, 40, 6, "cuda:0"
    T = burn + seq + n
    cap = 65536
    torch.cuda.synchronize()
    free_a, _ = torch.cuda.mem_get_info()
    rp = RNNReplay(cap, 7, 0.6, 0.4, 0, A, T, dev, dedup="plane", guard_units=(2 * T + n + 10) * R, units_per_slot=seq + n)
    torch.cuda.synchronize()
    free_b, _ = torch.cuda.mem_get_info()
    replay_bytes = free_a - free_b
    print("replay allocation at capacity 65,536 (plane units): %.2f GB" % (replay_bytes / 1e9))
    assert replay_bytes < 60e9
    ucap = C.c_int64()
    capi.check(capi.lib.rela_replay_dedup_info(rp.h, None, None, C.byref(ucap)), "dedup_info")
    on, tg = _lstm(A, 1, dev, "bf16x2"), _lstm(A, 2, dev, "bf16x2")
    eng = R2D2ActorEngine(R, K, A, n, 0.997, seq, burn, 0.9, rp, [0.0] * R, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    rows = torch.arange(R, device=dev, dtype=torch.int32)

    def plane_of(tick):  # [R, 84, 84]: bytes a function of (tick, row); bytes 0..3 carry tick and row
        x = (rows[:, None] * 7919 + tick * 104729 + torch.arange(PLANE, device=dev, dtype=torch.int32)[None, :] * 31) % 251
        p = x.to(torch.uint8).reshape(R, 84, 84)
        p[:, 0, 0] = tick & 255
        p[:, 0, 1] = (tick >> 8) & 255
        p[:, 0, 2] = rows & 255
        p[:, 0, 3] = rows >> 8
        return p

    stack = None
    zeros_r = np.zeros(R, np.float32)
    term = np.zeros(R, np.uint8)
    checked, t, batch = 0, 0, 64
    ring = int(1.25 * cap)
    while rp.num_add() <= ring + 4096 or t * R <= ucap.value + R:
        p = plane_of(t)
        stack = p[:, None].expand(R, 4, 84, 84).clone() if stack is None else torch.cat([stack[:, 1:], p[:, None]], 1)
        eng.next_obs_slot().copy_(stack)
        eng.act(on)
        eng.post_step(zeros_r, term, on, tg)
        if rp.size() > cap - 2 * R or (t % 40 == 39 and rp.size() >= batch):
            b, w = rp.sample(batch)
            s = b.obs["s"]  # [T, B, 4, 84, 84]
            pad = s.reshape(T, batch, -1).amax(-1) == 0  # [T, B] (the burn-in padding of each env's first sequence)
            tk = s[:, :, :, 0, 0].int() + 256 * s[:, :, :, 0, 1].int()
            rw = s[:, :, :, 0, 2].int() + 256 * s[:, :, :, 0, 3].int()
            newest = tk[:, :, 3]
            # every stack: planes of ticks newest-3..newest (clamped at 0) of one row; consecutive steps consecutive
            exp_tk = (newest[:, :, None] - 3 + torch.arange(4, device=dev)[None, None, :]).clamp(min=0)
            assert ((tk == exp_tk) | pad[:, :, None]).all()
            row_b = torch.where(pad, 0, rw[:, :, 0]).amax(0)
            assert ((rw == row_b[None, :, None]) | pad[:, :, None]).all()
            both = ~pad[1:] & ~pad[:-1]
            assert ((newest[1:] - newest[:-1] == 1) | ~both).all()
            assert (~pad).any(0).all()
            if t % 40 == 39:  # byte-exact rebuild of one sampled sequence's every plane
                bb = int(torch.randint(0, batch, (1,), device=dev, generator=g).item())
                r0 = int(row_b[bb])
                for tt in range(T):
                    if pad[tt, bb]:
                        continue
                    for k in range(4):
                        want = plane_of(int(tk[tt, bb, k]))[r0]
                        assert torch.equal(s[tt, bb, k], want)
            assert rp.debug_state()["dev_error"] == 0
            rp.update_priority(torch.rand(batch, device=dev, generator=g) + 0.1)
            checked += 1
        t += 1
    assert checked > 0 and rp.num_add() > ring and t * R > ucap.value
    eng.close()
    rp.close()


@pytest.fixture(scope="module")
def mods():
    sys.path.insert(0, os.path.join(ROOT, "rela_amd", "pybind"))
    import torch  # noqa: F401
    import rela
    import synth_atari

    return rela, synth_atari


@pytest.fixture
def dedup_env():
    def set_(mode, guard="4096"):
        if mode:
            os.environ["RELA_REPLAY_DEDUP"] = mode
            os.environ["RELA_REPLAY_DEDUP_GUARD"] = guard
        else:
            os.environ.pop("RELA_REPLAY_DEDUP", None)
            os.environ.pop("RELA_REPLAY_DEDUP_GUARD", None)
    yield set_
    os.environ.pop("RELA_REPLAY_DEDUP", None)
    os.environ.pop("RELA_REPLAY_DEDUP_GUARD", None)


class _Keep:
    """the `rela` module with RNNPrioritizedReplay instances kept for inspection after run_lockstep_r2d2 returns"""

    def __init__(self, rela):
        self._rela, self.replays = rela, []

    def __getattr__(self, name):
        return getattr(self._rela, name)

    def RNNPrioritizedReplay(self, *a):
        r = self._rela.RNNPrioritizedReplay(*a)
        self.replays.append(r)
        return r


def _r2d2_agent(C_):
    from e2e_lockstep import load_lstm_agent_params
    from rela_amd.pyrela.net import AtariLSTMNet
    from rela_amd.pyrela.r2d2 import R2D2Agent

    agent = R2D2Agent(lambda dev: AtariLSTMNet(dev, C_["num_action"]), "cpu", C_["multi_step"], C_["gamma"], C_["eta"],
                      C_["seq_len"], C_["burn_in"], 0)
    return load_lstm_agent_params(agent, C_)


@pytest.mark.parametrize("cfg", ["r2d2", "r2d2_c4"])
def test_seq_dedup_module_reproduces_reference_golden(mods, dedup_env, cfg):
    """RELA_REPLAY_DEDUP=stack through the drop-in module (RNNPrioritizedReplay + R2D2Actor): the lock-step run
    reproduces the REAL reference's recorded batches exactly as tests/test_e2e_gpu.py checks them, and the partition
    really is de-duplicated (it refuses the export a full-storage partition allows)."""
    from e2e_lockstep import CFG_R2D2, CFG_R2D2_C4, run_lockstep_r2d2

    rela, synth = mods
    C_ = CFG_R2D2 if cfg == "r2d2" else CFG_R2D2_C4
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "e2e_lockstep_%s.json" % cfg)))
    assert gold["cfg"] == C_
    dedup_env("stack")
    keep = _Keep(rela)
    rounds = run_lockstep_r2d2(keep, synth, _r2d2_agent(C_), "cuda:0", "cuda:0", C_, quiet=1.0 if cfg == "r2d2" else 3.0)
    tol = 1e-4 if cfg == "r2d2" else 2e-4
    assert len(rounds) == len(gold["expect"])
    for r, (got, exp) in enumerate(zip(rounds, gold["expect"])):
        for key in ("s_sum", "a", "terminal", "bootstrap", "legal_sum", "seq_len", "num_add", "size", "eps_sum"):
            assert got[key] == exp[key], (r, key)
        assert np.array_equal(np.float32(got["reward"]), np.float32(exp["reward"])), r
        np.testing.assert_allclose(got["h0_abs"], exp["h0_abs"], rtol=tol, atol=tol)
        np.testing.assert_allclose(got["c0_abs"], exp["c0_abs"], rtol=tol, atol=tol)
        np.testing.assert_allclose(got["weight"], exp["weight"], rtol=10 * tol, err_msg="IS weights, round %d" % r)
    (replay,) = keep.replays
    with pytest.raises(RuntimeError, match="cannot be exported"):
        replay.export_chunks()


def test_seq_dedup_module_plane_mode_matches_full_storage(mods, dedup_env):
    """RELA_REPLAY_DEDUP=plane through the module with a sliding-stack env: the same lock-step batches as full storage."""
    from e2e_lockstep import CFG_R2D2, run_lockstep_r2d2

    rela, synth = mods
    sliding = SimpleNamespace(SyntheticAtariEnv=lambda seed, eps, A, L: synth.SyntheticAtariEnv(seed, eps, A, L, True))
    out = []
    for mode in (None, "plane"):
        dedup_env(mode)
        keep = _Keep(rela)
        out.append(run_lockstep_r2d2(keep, sliding, _r2d2_agent(CFG_R2D2), "cuda:0", "cuda:0", CFG_R2D2))
        (replay,) = keep.replays
        if mode is None:
            replay.export_chunks()  # full storage exports
        else:
            with pytest.raises(RuntimeError, match="cannot be exported"):
                replay.export_chunks()
        del keep, replay
    assert out[0] == out[1]


def test_seq_dedup_export_refused():
    """rela_replay_export_ipc / _chunks refuse a sequence replay with de-duplicated stacks (RELA_EINVAL)."""
    from rela_amd import _capi as capi
    from rela_amd.replay import RNNReplay

    rp = RNNReplay(16, 1, 1.0, 1.0, 0, 4, 15, "cuda:0", dedup="stack", guard_units=64)
    assert capi.lib.rela_replay_dedup_steps(rp.h) == 15
    desc = capi.ReplayChunkDesc()
    fds = (C.c_int * capi.IPC_MAX_FDS)()
    assert capi.lib.rela_replay_export_chunks(rp.h, C.byref(desc), fds, capi.IPC_MAX_FDS) == capi.EINVAL
    assert b"cannot be exported" in capi.lib.rela_last_error()
    ipc = capi.ReplayIpcDesc()
    assert capi.lib.rela_replay_export_ipc(rp.h, C.byref(ipc)) == capi.EINVAL
    from rela_amd.parallel import _export_desc

    with pytest.raises(ValueError, match="cannot be exchanged"):
        _export_desc(rp.h)
    rp.close()


def test_seq_dedup_r2d2_training_entry_point_runs(capsys, dedup_env):
    """main.py --algo r2d2 on 2 threads x 4 envs with RELA_REPLAY_DEDUP=plane on the sliding synthetic env."""
    from rela_amd.pyrela import main as entry

    dedup_env("plane")
    os.environ["RELA_SYNTH_SLIDING"] = "1"
    try:
        args = entry.parse_args(["--algo", "r2d2", "--num_thread", "2", "--num_game_per_thread", "4", "--batchsize", "8",
                                 "--epoch_len", "40", "--num_epoch", "2", "--burn_in_frames", "16",
                                 "--replay_buffer_size", "64", "--episode_len", "30", "--actor_sync_freq", "3",
                                 "--seq_len", "8", "--seq_burn_in", "4", "--priority_exponent", "0.9",
                                 "--importance_exponent", "0.6"])
        hist = entry.train(args)
    finally:
        os.environ.pop("RELA_SYNTH_SLIDING", None)
    out = capsys.readouterr().out
    assert "Speed: train: " in out
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) for h in hist)
    assert hist[-1]["act"] > 0 and max(h["buffer_add"] for h in hist) > 0
