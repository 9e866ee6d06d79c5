"""Device-resident envs: the env layer of an actor engine that never leaves the GPU.

`DeviceCatchEnv` is the Python handle on rela_catch_* (csrc/catch_env.hip over csrc/catch_game.h): `rows` games of Catch
whose state lives in HBM and whose frame stacks are rendered straight into an actor engine's observation slot.

An evaluation engine (replay=None) acts on one slot, so a tick is one fused launch:

    env.reset(eng.next_obs_slot())
    action = eng.act(online)
    reward, terminal = env.step(action, eng.next_obs_slot())

An engine WITH a replay keeps all n + 1 history slots live during post_step() -- the slot of the next observation still
holds the oldest stack of the transition being inserted -- and post_step() takes the reward.  There the tick is

    action = eng.act(online)
    reward, terminal = env.step(action)             # state, reward, terminal: no frame is written
    eng.post_step(reward, terminal, online, target)
    env.render(eng.next_obs_slot())                 # the slot post_step() has just released
"""
import ctypes as C

import numpy as np
import torch

from . import _capi as capi
from .engine import dev_view

STATE_COLUMNS = ("lcg", "px", "bx", "by", "dx", "steps", "ep_return", "bad_actions")


class DeviceCatchEnv:
    """rows games of Catch on `device`; row r plays the game seeded seed + r (= synth_atari.CatchEnv(seed + r))."""

    def __init__(self, rows, num_action, episode_len, seed, device="cuda:0"):
        self.rows, self.num_action, self.episode_len = rows, num_action, episode_len
        self.device = torch.device(device)
        h = C.c_void_p()
        capi.check(capi.lib.rela_catch_create(C.byref(h), rows, num_action, episode_len, seed, self.device.index or 0),
                   "rela_catch_create")
        self.h = h
        self.reward = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.terminal = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        self._stats = dev_view(capi.lib.rela_catch_stats_dev(h), (4, rows), torch.int32, self.device)
        self._host = None

    def close(self):
        if getattr(self, "h", None):
            capi.lib.rela_catch_destroy(self.h)
            self.h = None

    def __del__(self):
        if capi is not None and getattr(capi, "lib", None) is not None:  # module globals die first at exit
            self.close()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _slot_ptr(self, slot):
        if slot.dtype != torch.uint8 or slot.numel() != self.rows * 4 * 84 * 84 or not slot.is_contiguous() or \
                slot.device != self.device:
            raise ValueError("DeviceCatchEnv: the slot must be a contiguous u8 [%d, 4, 84, 84] tensor on %s" % (
                self.rows, self.device))
        return C.c_void_p(slot.data_ptr())

    def reset(self, slot):
        """reset() of every row; writes the first observations into `slot` (engine.next_obs_slot())."""
        capi.check(capi.lib.rela_catch_reset(self.h, self._slot_ptr(slot), self._stream()), "rela_catch_reset")

    def step(self, action, slot=None):
        """Steps every row with action (cuda i64 [rows]) -> (reward f32 [rows], terminal u8 [rows]), device tensors this
        env owns and overwrites with the next step.  With `slot` the same launch writes the next observations into it;
        without, render(slot) does that later (an engine with a replay: after post_step())."""
        if action.dtype != torch.int64 or action.numel() != self.rows or action.device != self.device:
            raise ValueError("DeviceCatchEnv.step: action must be a cuda int64 tensor of %d elements" % self.rows)
        self._keep = action if action.is_contiguous() else action.contiguous()
        capi.check(capi.lib.rela_catch_step(self.h, C.c_void_p(self._keep.data_ptr()),
                                            self._slot_ptr(slot) if slot is not None else None,
                                            C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.terminal.data_ptr()),
                                            self._stream()), "rela_catch_step")
        return self.reward, self.terminal

    def render(self, slot):
        """Writes the current observations into `slot`."""
        capi.check(capi.lib.rela_catch_render(self.h, self._slot_ptr(slot), self._stream()), "rela_catch_render")

    def step_host(self, action, slot=None):
        """step(), then page-locked numpy copies of reward and terminal after a synchronise: what a shard whose
        bookkeeping branches on the host takes (R2D2ActorEngine.post_step).  -> (reward, terminal, reward_np, terminal_np)"""
        reward, terminal = self.step(action, slot)
        if self._host is None:
            self._host = (torch.zeros(self.rows, dtype=torch.float32).pin_memory(),
                          torch.zeros(self.rows, dtype=torch.uint8).pin_memory())
        self._host[0].copy_(reward, non_blocking=True)
        self._host[1].copy_(terminal, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return reward, terminal, self._host[0].numpy(), self._host[1].numpy()

    def stats_dev(self):
        """int32 [4, rows] on the device: episodes, return_sum, last_return, last_len of every row (a live view)."""
        return self._stats

    def episode_stats(self):
        """Totals over the rows as Python ints (int64 sums: no overflow) plus copies of the per-row tensors."""
        st = self._stats.clone()
        episodes, return_sum = int(st[0].sum(dtype=torch.int64)), int(st[1].sum(dtype=torch.int64))
        return {"episodes": episodes, "return_sum": return_sum,
                "mean_return": return_sum / episodes if episodes else float("nan"),
                "rows": {"episodes": st[0], "return_sum": st[1], "last_return": st[2], "last_len": st[3]}}

    def state(self):
        """int32 numpy [rows, 8]: the columns STATE_COLUMNS; synchronises."""
        out = np.zeros((self.rows, 8), np.int32)
        capi.check(capi.lib.rela_catch_debug_state(self.h, out.ctypes.data_as(C.c_void_p)), "rela_catch_debug_state")
        return out
