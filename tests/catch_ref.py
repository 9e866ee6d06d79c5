"""Catch on 84x84 restated in plain Python integers, from the specification (not from rela_amd/csrc/catch_game.h): the
reference the host env, the CPU shim and the device env are compared with.

  LCG        state <- (state * 1664525 + 1013904223) mod 2^32, the draw is the new state; seeded state = (seed mod 2^32) *
             2654435761 + 40503 (mod 2^32)
  spawn      bx = 4 * ((draw >> 24) % 21); dx = 4 * ((draw >> 24) % 3 - 1); by = 0        (two draws, in this order)
  reset      steps = 0, ep_return = 0; px = 4 * ((draw >> 24) % 19); spawn; the history is four times (px, bx, by)
  step(a)    paddle: px = clamp(px + 4 * (a % 3 - 1), 0, 72); ball: bx += dx, reflected at 0 and 80 with dx negated;
             by += 4; landed (by >= 80): reward +1 if bx + 3 >= px and bx <= px + 11 else -1, then spawn; the history
             takes (px, bx, by); steps += 1; ep_return += reward; terminal = steps >= episode_len
  pixels     255 inside the ball's 4 x 4 square at (by, bx), else 170 inside the paddle's 3 x 12 bar at (80, px), else 0;
             plane 3 is the newest history entry
"""
import numpy as np

M32 = 0xFFFFFFFF


class CatchRef:
    """One game.  `auto_reset=True` gives the vector semantics of the device env: a step that ends the episode returns
    terminal with its reward and the game is already reset (the observation is the new episode's first); the finished
    episode's return and length go to the statistics.  A bad action (outside [0, num_action)) then leaves the game as it
    is and counts; with auto_reset=False (the host env) it raises IndexError."""

    def __init__(self, seed, num_action=18, episode_len=200, auto_reset=False):
        self.lcg = ((seed & M32) * 2654435761 + 40503) & M32
        self.num_action, self.episode_len, self.auto_reset = num_action, episode_len, auto_reset
        self.px = self.bx = self.by = self.dx = self.steps = self.ep_return = 0
        self.bad_actions = 0
        self.hist = [(0, 0, 0)] * 4
        self.terminal = True
        self.episodes = self.return_sum = self.last_return = self.last_len = 0

    def _next(self):
        self.lcg = (self.lcg * 1664525 + 1013904223) & M32
        return self.lcg

    def _spawn(self):
        self.bx = 4 * ((self._next() >> 24) % 21)
        self.dx = 4 * ((self._next() >> 24) % 3 - 1)
        self.by = 0

    def reset(self):
        self.steps = 0
        self.ep_return = 0
        self.terminal = False
        self.px = 4 * ((self._next() >> 24) % 19)
        self._spawn()
        self.hist = [(self.px, self.bx, self.by)] * 4
        return self.obs()

    def step(self, a):
        """-> (reward, terminal)"""
        a = int(a)
        if a < 0 or a >= self.num_action:
            if not self.auto_reset:
                raise IndexError("action out of range")
            self.bad_actions += 1
            return 0, False
        self.px = min(max(self.px + 4 * (a % 3 - 1), 0), 72)
        self.bx += self.dx
        if self.bx < 0:
            self.bx, self.dx = -self.bx, -self.dx
        if self.bx > 80:
            self.bx, self.dx = 160 - self.bx, -self.dx
        self.by += 4
        reward = 0
        if self.by >= 80:
            reward = 1 if (self.bx + 3 >= self.px and self.bx <= self.px + 11) else -1
            self._spawn()
        self.hist = self.hist[1:] + [(self.px, self.bx, self.by)]
        self.steps += 1
        self.ep_return += reward
        terminal = self.steps >= self.episode_len
        self.terminal = terminal
        if terminal and self.auto_reset:
            self.episodes += 1
            self.return_sum += self.ep_return
            self.last_return, self.last_len = self.ep_return, self.steps
            self.reset()
        return reward, terminal

    def obs(self):
        """uint8 [4, 84, 84]"""
        out = np.zeros((4, 84, 84), np.uint8)
        for k, (px, bx, by) in enumerate(self.hist):
            out[k, 80:83, px:px + 12] = 170
            out[k, by:by + 4, bx:bx + 4] = 255
        return out

    def state(self):
        """the columns of DeviceCatchEnv.state(): lcg bits as int32, px, bx, by, dx, steps, ep_return, bad_actions"""
        lcg = self.lcg - (1 << 32) if self.lcg >= (1 << 31) else self.lcg
        return [lcg, self.px, self.bx, self.by, self.dx, self.steps, self.ep_return, self.bad_actions]


class CatchRefVec:
    """rows games with auto-reset, row r seeded seed + r: the reference of DeviceCatchEnv."""

    def __init__(self, rows, num_action, episode_len, seed):
        self.games = [CatchRef(seed + r, num_action, episode_len, auto_reset=True) for r in range(rows)]

    def reset(self):
        return np.stack([g.reset() for g in self.games])

    def step(self, actions):
        out = [g.step(a) for g, a in zip(self.games, actions)]
        reward = np.array([o[0] for o in out], np.float32)
        terminal = np.array([o[1] for o in out], np.uint8)
        return reward, terminal

    def obs(self):
        return np.stack([g.obs() for g in self.games])

    def state(self):
        return np.array([g.state() for g in self.games], np.int32)

    def stats(self):
        """int32 [4, rows]: episodes, return_sum, last_return, last_len"""
        return np.array([[g.episodes for g in self.games], [g.return_sum for g in self.games],
                         [g.last_return for g in self.games], [g.last_len for g in self.games]], np.int32)


def walk_policy(game):
    """the action that walks the paddle towards bx - 4 (0 left, 1 stay, 2 right)"""
    target = game.bx - 4
    return 0 if game.px > target else (2 if game.px < target else 1)
