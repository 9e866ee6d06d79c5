"""Indexed-colour screens (ALEInterface::getScreen: one palette index per pixel, a 256-entry RGB table per env) on the
host: synth_atari.screen_features_indexed, the indexed synthetic env, and the register budget of the kernel (no GPU
needed).

The frame computeFeature sees is max(pal[ia], pal[ib]) per channel, so the reference is always the RGB restatement
synth_atari.screen_features on the expanded screens pal[ia], pal[ib], and everything is exact equality."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_atari_screen_cpu import edge_pairs  # noqa: E402  (puts rela_amd/pybind on sys.path)


@pytest.fixture(scope="module")
def synth():
    import rela  # noqa: F401  (registers rela.Env)
    import synth_atari

    return synth_atari


def indexed_pairs(H=210, W=160, n=40, seed=0):
    """n x (ia, ib, pal): uniform indices in 0..255 and a uniform random palette each"""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8),
             rng.integers(0, 256, (256, 3), dtype=np.uint8)) for _ in range(n)]


def edge_indexed(H, W):
    """the edge_pairs pictures with the two-entry palette {0: 0, 1: 255}; their one other value, the G = 200 row, gets
    index 2 = (0, 200, 0).  Returns (ia, ib, pal) triples whose expansion IS edge_pairs(H, W)."""
    pal = np.zeros((256, 3), np.uint8)
    pal[1] = 255
    pal[2] = (0, 200, 0)
    out = []
    for a, b in edge_pairs(H, W):
        tr = []
        for s in (a, b):
            idx = np.zeros((H, W), np.uint8)
            idx[(s == 255).all(axis=2)] = 1
            idx[(s[..., 1] == 200) & (s[..., 0] == 0)] = 2
            assert np.array_equal(pal[idx], s)
            tr.append(idx)
        out.append((tr[0], tr[1], pal))
    return out


def features_indexed(synth, triples):
    return np.stack([synth.screen_features_indexed(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(p)).numpy()
                     for a, b, p in triples])


def features_expanded(synth, triples):
    return np.stack([synth.screen_features(torch.from_numpy(p[a]), torch.from_numpy(p[b])).numpy() for a, b, p in triples])


@pytest.mark.parametrize("shape", [(210, 160), (250, 160)])
def test_indexed_equals_rgb_restatement_random(synth, shape):
    tr = indexed_pairs(*shape)
    got, ref = features_indexed(synth, tr), features_expanded(synth, tr)
    assert got.shape == (40, 84, 84) and got.dtype == np.uint8
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert len(np.unique(got)) > 50  # not a constant picture


@pytest.mark.parametrize("shape", [(210, 160), (250, 160)])
def test_indexed_equals_rgb_restatement_edge_pictures(synth, shape):
    tr = edge_indexed(*shape)
    got, ref = features_indexed(synth, tr), features_expanded(synth, tr)
    assert np.array_equal(got, ref)
    assert (got[0] == 0).all() and (got[1] == 255).all()


@pytest.mark.parametrize("shape", [(210, 160), (250, 160)])
def test_indexed_special_palettes(synth, shape):
    """an all-zero and an all-255 palette, and one where only even indices (ALE's) are non-zero"""
    rng = np.random.default_rng(5)
    ia, ib, pal = indexed_pairs(*shape, n=1, seed=6)[0]
    even = pal.copy()
    even[1::2] = 0
    tr = [(ia, ib, np.zeros((256, 3), np.uint8)), (ia, ib, np.full((256, 3), 255, np.uint8)), (ia, ib, even),
          (ia & 0xFE, ib & 0xFE, even), (rng.integers(0, 256, shape, dtype=np.uint8), ib, even)]
    got, ref = features_indexed(synth, tr), features_expanded(synth, tr)
    assert np.array_equal(got, ref)
    assert (got[0] == 0).all() and (got[1] == 255).all()


def test_indexed_refuses_bad_arguments(synth):
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError):
        synth.screen_features_indexed(z(1, 160), z(1, 160), z(256, 3))
    with pytest.raises(ValueError):
        synth.screen_features_indexed(z(210, 160), z(210, 161), z(256, 3))
    with pytest.raises(ValueError):
        synth.screen_features_indexed(z(210, 160), z(210, 160), z(255, 3))
    with pytest.raises(ValueError):
        synth.screen_features_indexed(z(210, 160, 3), z(210, 160, 3), z(256, 3))


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_indexed_env_draws_the_rgb_envs_picture(synth, seed):
    """70 steps across an episode boundary (episodes of 30): the indexed host env returns the RGB host env's obs["s"],
    rewards and terminals, and palette()[screens()] is the RGB env's screens() at every step; the five-argument
    constructor call still means RGB."""
    L = 30
    rgb = synth.SyntheticScreenEnv(seed, 0.0, 18, L, False)
    idx = synth.SyntheticScreenEnv(seed, 0.0, 18, L, False, indexed=True)
    dev = synth.SyntheticScreenEnv(seed, 0.0, 18, L, True, True)
    assert isinstance(dev, synth.SyntheticScreenEnvDevice) and not isinstance(idx, synth.SyntheticScreenEnvDevice)
    pal = idx.palette().numpy()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8 and (pal[16:] == 0).all()
    assert np.array_equal(pal[8:16], 255 - pal[:8])
    assert np.array_equal(pal, dev.palette().numpy())
    act = {"a": torch.zeros(1, dtype=torch.int64)}
    rng = np.random.default_rng(seed)
    resets = 0
    for t in range(70 + 3):
        if t == 0 or rgb.terminated():
            assert t == 0 or (idx.terminated() and dev.terminated())
            o = [e.reset() for e in (rgb, idx, dev)]
            resets += 1
        else:
            act["a"][0] = int(rng.integers(0, 18))
            res = [e.step(act) for e in (rgb, idx, dev)]
            assert res[0][1:] == res[1][1:] == res[2][1:], t  # reward, terminal
            o = [r[0] for r in res]
        assert torch.equal(o[0]["s"], o[1]["s"]), t
        scr = idx.screens().numpy()
        assert scr.shape == (2, 210, 160) and np.array_equal(scr, dev.screens().numpy())
        assert np.array_equal(pal[scr], rgb.screens().numpy()), t
    assert resets == 3
    assert rgb.get_episode_reward() == idx.get_episode_reward() == dev.get_episode_reward()


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark key: int}} of csrc/atari_screen.hip's kernels"""
    from rela_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here")
    obj = str(tmp_path_factory.mktemp("screenres") / "atari_screen_dev.o")
    cmd = [hipcc] + b.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                   os.path.join(b.CSRC, "atari_screen.hip"), "-o", obj]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_indexed_kernels_no_scratch_no_spills(resources):
    ks = {n: v for n, v in resources.items() if "atari_features_indexed_kernel" in n}
    assert len(ks) == 2, sorted(resources)  # the 16-byte-load and the byte-load instantiation
    for name, v in ks.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
