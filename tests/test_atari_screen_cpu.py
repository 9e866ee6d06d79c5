"""GameState::computeFeature (atari/game_state.h:53-82,122-133) restated on the host: synth_atari.screen_features and the
raw-screen synthetic env (no GPU needed).

The reference arithmetic is torch on the CPU running the reference's own ops: bilinear interpolation with
align_corners=True of max(a, b).float() / 255, the gray sum, * 255 and the cast to uint8.  Its order of operations and
contraction depend on the build, so the restatement (a fixed float32 recipe, csrc/atari_screen.h) need not be
bit-identical to it: every pixel must be within 1 and at most 1e-3 of all pixels may differ."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYBIND = os.path.join(ROOT, "rela_amd", "pybind")
if PYBIND not in sys.path:
    sys.path.insert(0, PYBIND)

MAX_DIFF, MAX_FRAC = 1, 1e-3


@pytest.fixture(scope="module")
def synth():
    import rela  # noqa: F401  (registers rela.Env)
    import synth_atari

    return synth_atari


def torch_feature(a, b):
    """the reference's ops: [H,W,3] u8 x2 -> [84,84] u8"""
    H, W = a.shape[:2]
    x = torch.from_numpy(np.maximum(a, b)).float().permute(2, 0, 1).contiguous() / 255.0
    x = F.interpolate(x.view(1, 3, H, W), size=(84, 84), mode="bilinear", align_corners=True).view(3, 84, 84)
    s = 0.21 * x[0] + 0.72 * x[1] + 0.07 * x[2]
    return (s * 255.0).to(torch.uint8).numpy()


def screen_pairs(H=210, W=160, n=40, seed=0):
    """n pairs: even k uniform-random, odd k 8-colour palette screens with 10-pixel blocks"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 2 == 0:
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            pal = rng.integers(0, 256, (8, 3), dtype=np.uint8)
            hb, wb = -(-H // 10), -(-W // 10)
            a = pal[rng.integers(0, 8, (hb, wb))].repeat(10, 0).repeat(10, 1)[:H, :W]
            b = pal[rng.integers(0, 8, (hb, wb))].repeat(10, 0).repeat(10, 1)[:H, :W]
        out.append((np.ascontiguousarray(a), np.ascontiguousarray(b)))
    return out


def edge_pairs(H, W):
    """all-0, all-255, one saturated pixel at each corner (in a and in b), the first and the last source row lit"""
    z = np.zeros((H, W, 3), np.uint8)
    out = [(z, z), (np.full_like(z, 255), np.full_like(z, 255))]
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        p = z.copy()
        p[y, x] = 255
        out += [(p, z), (z, p)]
    for y in (0, H - 1):
        p = z.copy()
        p[y] = 255
        q = z.copy()
        q[y, :, 1] = 200
        out += [(p, z), (z, q)]
    return out


def cap_check(got, ref, what):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    frac = float((d != 0).mean())
    print("%s: max |diff| %d, differing pixels %d of %d (%.2e)" % (what, d.max(), (d != 0).sum(), d.size, frac))
    assert d.max() <= MAX_DIFF, what
    assert frac <= MAX_FRAC, what


def features(synth, pairs):
    return np.stack([synth.screen_features(torch.from_numpy(a), torch.from_numpy(b)).numpy() for a, b in pairs])


@pytest.mark.parametrize("shape", [(210, 160), (250, 160)])
def test_screen_features_within_cap_of_torch(synth, shape):
    H, W = shape
    pairs = screen_pairs(H, W)
    got = features(synth, pairs)
    ref = np.stack([torch_feature(a, b) for a, b in pairs])
    assert got.shape == (40, 84, 84) and got.dtype == np.uint8
    cap_check(got, ref, "40 pairs %dx%d" % shape)


@pytest.mark.parametrize("shape", [(210, 160), (250, 160)])
def test_screen_features_edge_cases(synth, shape):
    H, W = shape
    pairs = edge_pairs(H, W)
    got = features(synth, pairs)
    ref = np.stack([torch_feature(a, b) for a, b in pairs])
    cap_check(got, ref, "edge cases %dx%d" % shape)
    assert (got[0] == 0).all() and (got[1] == 255).all()
    # each corner pixel reaches exactly its corner of the output (align_corners), in a and in b alike
    for i, (y, x) in enumerate(((0, 0), (0, 83), (83, 0), (83, 83))):
        for j in (2 + 2 * i, 3 + 2 * i):
            assert np.unravel_index(np.argmax(got[j]), got[j].shape) == (y, x) and got[j][y, x] >= 254, (i, j)


def test_screen_features_is_the_max_of_the_pair(synth):
    a, b = screen_pairs(n=2)[0]
    m = np.maximum(a, b)
    ab = features(synth, [(a, b)])[0]
    assert np.array_equal(ab, features(synth, [(b, a)])[0])
    assert np.array_equal(ab, features(synth, [(m, m)])[0])


def test_screen_features_refuses_bad_shapes(synth):
    with pytest.raises(ValueError):
        synth.screen_features(torch.zeros(1, 160, 3, dtype=torch.uint8), torch.zeros(1, 160, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        synth.screen_features(torch.zeros(210, 513, 3, dtype=torch.uint8), torch.zeros(210, 513, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        synth.screen_features(torch.zeros(210, 160, 3, dtype=torch.uint8), torch.zeros(210, 161, 3, dtype=torch.uint8))


def test_screen_env_host_mode_stacks_frames_like_compute_feature(synth):
    """device_features=False: obs["s"] is computeFeature's four-plane deque of screen_features(current, previous) --
    all four planes after reset(), slide by one per step()."""
    env = synth.SyntheticScreenEnv(3, 0.0, 18, 5, False)
    twin = synth.SyntheticScreenEnv(3, 0.0, 18, 5, True)
    assert not isinstance(env, synth.SyntheticScreenEnvDevice) and isinstance(twin, synth.SyntheticScreenEnvDevice)
    act = {"a": torch.zeros(1, dtype=torch.int64)}
    stack = None
    rng = np.random.default_rng(1)
    for t in range(12):
        if t == 0 or env.terminated():
            s = env.reset()["s"].numpy().copy()
            twin.reset()
            r = rt = 0.0
        else:
            act["a"][0] = int(rng.integers(0, 18))
            obs, r, _ = env.step(act)
            _, rt, _ = twin.step(act)
            s = obs["s"].numpy().copy()
        scr = env.screens().numpy()
        assert np.array_equal(scr, twin.screens().numpy()) and r == rt  # the same screens and rewards in both modes
        f = synth.screen_features(torch.from_numpy(scr[0]), torch.from_numpy(scr[1])).numpy()
        stack = np.stack([f] * 4) if (stack is None or t % 6 == 0) else np.concatenate([stack[1:], f[None]])
        assert np.array_equal(s, stack), t
    assert env.get_episode_reward() == twin.get_episode_reward()


def test_screen_env_frames_depend_on_actions(synth):
    act = {"a": torch.zeros(1, dtype=torch.int64)}
    envs = [synth.SyntheticScreenEnv(9, 0.0, 18, 50, False) for _ in range(2)]
    for e in envs:
        e.reset()
    for k, e in enumerate(envs):
        act["a"][0] = 0 if k == 0 else 8
        for _ in range(3):
            e.step(act)
    assert not np.array_equal(envs[0].screens().numpy(), envs[1].screens().numpy())


def test_mixed_vector_env_raises_at_first_reset(synth):
    """a VectorEnv with a screen env and a plain env refuses at its first reset() (raised through Context)."""
    import time

    import rela

    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet

    agent = ApexAgent(lambda: AtariFFNet(18), 3, 0.99)
    locker = rela.ModelLocker([agent], "cpu")
    replay = rela.FFPrioritizedReplay(64, 1, 1.0, 1.0, 0)
    vec = rela.VectorEnv()
    vec.append(synth.SyntheticScreenEnv(1, 0.0, 18, 10, True))
    vec.append(synth.SyntheticAtariEnv(2, 0.0, 18, 10))
    ctx = rela.Context()
    ctx.push_env_thread(rela.BasicThreadLoop(rela.DQNActor(locker, 3, 2, 0.99, replay), vec, False))
    ctx.start()
    t0 = time.time()
    with pytest.raises(RuntimeError, match="ScreenEnvs"):
        while not ctx.terminated():
            assert time.time() - t0 < 60
            time.sleep(0.01)
