"""State guards of the actor shards' C ABI (rela_apex_actor_*, rela_r2d2_actor_*) that live in the code both shards
share (csrc/actor_shard.h): every refusal returns its documented code and names its own entry point in
rela_last_error().  The smallest shapes that reach them: 4 rows in groups of 2, 6 actions, multi_step 2 (R2D2:
seq_len 4, burn_in 2)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, K, A, N, SEQ, BURN = 4, 2, 6, 2, 4, 2
T = BURN + SEQ + N
DEV = "cuda:0"
KINDS = ("apex", "r2d2")


@pytest.fixture(scope="module")
def nets():
    import torch

    from rela_amd.engine import FFNetHandle, LSTMNetHandle
    from synth import synth_lstm_params, synth_params

    out = {}
    for kind, cls, params in (("apex", FFNetHandle, synth_params), ("r2d2", LSTMNetHandle, synth_lstm_params)):
        pair = []
        for seed in (11, 12):
            h = cls(A, DEV)
            h.load_state_dict({k: torch.from_numpy(v) for k, v in params(A, seed).items()})
            pair.append(h)
        out[kind] = pair
    yield out
    for pair in out.values():
        for h in pair:
            h.close()


class _Shard:
    """a shard made through the bare ABI (the engines of rela_amd.engine call set_dedup themselves)"""

    def __init__(self, kind, replay=None):
        from rela_amd import _capi as capi

        self.capi, self.kind, self.prefix = capi, kind, "rela_%s_actor_" % kind
        h = C.c_void_p()
        rh = replay.h if replay is not None else None
        if kind == "apex":
            rc = capi.lib.rela_apex_actor_create(C.byref(h), R, K, A, N, 0.997, rh, 1, 0)
        else:
            rc = capi.lib.rela_r2d2_actor_create(C.byref(h), R, K, A, N, 0.997, SEQ, BURN, 0.9, rh, 1, 0)
        capi.check(rc, self.prefix + "create")
        self.h = h

    def fn(self, name):
        return getattr(self.capi.lib, self.prefix + name)

    def call(self, name, *args):
        return self.fn(name)(self.h, *args)

    def refused(self, code, name, *args, match=None):
        """the call returns `code` and the message starts with the entry point's own name"""
        rc = self.call(name, *args)
        msg = self.capi.lib.rela_last_error().decode()
        assert rc == code, (self.prefix + name, rc, msg)
        assert msg.startswith(self.prefix + name + ":"), msg
        if match:
            assert match in msg, msg

    def act(self, online):
        out = C.c_void_p()
        self.capi.check(self.call("act", online.h, None, None, None, None, C.byref(out), None), self.prefix + "act")

    def post_step(self, online, target):
        r, t, ins = np.zeros(R, np.float32), np.zeros(R, np.uint8), C.c_int(0)
        args = [r.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)] + ([0] if self.kind == "apex" else [])
        return args + [online.h, target.h, 0, C.byref(ins), None]

    def close(self):
        self.fn("destroy")(self.h)


def _replay(kind, dedup):
    from rela_amd.replay import FFReplay, RNNReplay

    if kind == "apex":
        return FFReplay(16, 7, 0.6, 0.4, 0, A, DEV, dedup=dedup, guard_units=(N + 8) * R)
    return RNNReplay(16, 7, 0.6, 0.4, 0, A, T, DEV, dedup=dedup, guard_units=(2 * T + N + 10) * R, units_per_slot=SEQ + N)


@pytest.mark.parametrize("kind", KINDS)
def test_slide_stacks_needs_a_staged_plane_and_a_first_whole_observation(kind):
    from rela_amd import _capi as capi

    sh = _Shard(kind)
    restart = np.zeros(R, np.uint8).ctypes.data_as(C.c_void_p)
    sh.refused(capi.ESTATE, "slide_stacks", restart, None, match="no plane was staged")
    assert sh.call("plane_stage")
    sh.refused(capi.ESTATE, "slide_stacks", restart, None, match="uploaded whole")
    sh.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_reuse_takes_0_1_2(kind):
    from rela_amd import _capi as capi

    sh = _Shard(kind)
    for on in (3, -1):
        sh.refused(capi.EINVAL, "set_reuse", on)
    for on in (0, 1, 2):
        assert sh.call("set_reuse", on) == capi.OK
    sh.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_dedup_needs_a_replay(kind):
    from rela_amd import _capi as capi

    sh = _Shard(kind)
    sh.refused(capi.EINVAL, "set_dedup", 1)
    sh.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_dedup_once_and_before_the_first_act(kind, nets):
    from rela_amd import _capi as capi

    replay = _replay(kind, "stack")
    sh = _Shard(kind, replay)
    assert sh.call("set_dedup", 1) == capi.OK, capi.lib.rela_last_error()
    sh.refused(capi.ESTATE, "set_dedup", 1)
    sh.close()
    sh = _Shard(kind, replay)
    sh.act(nets[kind][0])  # an act() with no post_step(): no tick was stored yet, the call is late all the same
    sh.refused(capi.ESTATE, "set_dedup", 1)
    sh.close()
    replay.close()


@pytest.mark.parametrize("kind", KINDS)
def test_post_step_needs_a_replay_and_an_act(kind, nets):
    from rela_amd import _capi as capi

    online, target = nets[kind]
    sh = _Shard(kind)  # evaluation shard
    sh.act(online)
    sh.refused(capi.ESTATE, "post_step", *sh.post_step(online, target), match="no replay")
    sh.close()
    replay = _replay(kind, None)
    sh = _Shard(kind, replay)
    sh.refused(capi.ESTATE, "post_step", *sh.post_step(online, target), match="no act()")
    sh.close()
    replay.close()


@pytest.mark.parametrize("kind", KINDS)
def test_null_handle_gives_null_and_zero(kind):
    from rela_amd import _capi as capi

    for name in ("obs_slot", "plane_stage", "screen_stage", "palette_stage"):
        assert getattr(capi.lib, "rela_%s_actor_%s" % (kind, name))(None) is None
    assert getattr(capi.lib, "rela_%s_actor_num_act" % kind)(None) == 0
