"""act_kernel and td_kernel (rela_amd/csrc/agent_ops.hip) against the exact references of tests/agent_ops_ref.py, through the
C ABI, at the smallest shapes that reach every path of the launchers (256 / 1,024 threads, one and several passes of the row
loop, ragged last groups, one group), on the role tables whose properties tests/test_agent_ops_ref_cpu.py asserts; the draws
under several seeds and counter offsets; the batching independence the kernel's comment claims; and one run through each
actor shard with eps > 0, which pins the counter schedule act_calls * R + row, the seed, and the use of each tick's own eps
and legal mask.  Every assertion is exact: nothing here has a tolerance, and nothing is statistical."""
import ctypes as C
import functools

import numpy as np
import pytest

import agent_ops_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SHAPE_IDS = ["n%d-group%d-A%d" % s for s in R.SHAPES]


@functools.lru_cache(maxsize=None)
def case_of(shape):
    return R.role_cases(*shape)


@functools.lru_cache(maxsize=None)
def truth_of(shape):
    return R.run_case(case_of(shape))


def run_act(q, legal, eps, group, seed, offset):
    """rela_apex_act_from_q -> int64[n] on the host (eps None: a null pointer, which the kernel reads as all zero)"""
    import torch

    from gpu_util import cur_stream, dev, ptr
    from rela_amd import _capi as capi

    n, A = q.shape
    d_q, d_legal, d_eps = dev(np.array(q)), dev(np.array(legal)), (dev(np.array(eps, F)) if eps is not None else None)
    d_act = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    capi.check(capi.lib.rela_apex_act_from_q(n, A, group, ptr(d_q), ptr(d_legal), ptr(d_eps), seed, offset, ptr(d_act),
                                             cur_stream()), "rela_apex_act_from_q")
    return d_act.cpu().numpy()


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_role_tables_exact(shape):
    """the actions under the table's eps, the greedy column (eps = 0, as an array and as a null pointer) and both outputs
    of rela_apex_td_from_q, bit for bit"""
    import torch

    from gpu_util import cur_stream, dev, ptr
    from rela_amd import _capi as capi

    n, group, A = shape
    case, want = case_of(shape), truth_of(shape)
    got = run_act(case["q"], case["legal"], case["eps"], group, case["seed"], case["offset"])
    bad = np.flatnonzero(got != want["action"])
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want["action"][bad[:8]], [k for k, v in case["roles"].items() if bad[0] in v])
    for eps in (np.zeros(n, F), None):
        got = run_act(case["q"], case["legal"], eps, group, case["seed"], case["offset"])
        bad = np.flatnonzero(got != want["greedy"])
        assert len(bad) == 0, (bad[:8], got[bad[:8]], want["greedy"][bad[:8]], [k for k, v in case["roles"].items() if bad[0] in v])
    td = case["td"]
    d = {k: dev(v.copy()) for k, v in td.items() if isinstance(v, np.ndarray)}  # (the shared tables are read-only)
    d_qno, d_legal = dev(case["q"].copy()), dev(case["legal"].copy())
    d_td = torch.full((n,), float("nan"), device="cuda")
    d_pr = torch.full((n,), float("nan"), device="cuda")
    capi.check(capi.lib.rela_apex_td_from_q(n, A, group, ptr(d["q"]), ptr(d_qno), ptr(d["qnt"]), ptr(d_legal), ptr(d["action"]),
                                            ptr(d["reward"]), ptr(d["bootstrap"]), C.c_float(td["gamma_n"]), ptr(d_td),
                                            ptr(d_pr), cur_stream()), "rela_apex_td_from_q")
    for key, out in (("td", d_td), ("prio", d_pr)):
        bad = np.flatnonzero(out.cpu().numpy().view(np.uint32) != want[key].view(np.uint32))
        assert len(bad) == 0, (key, bad[:8], [k for k, v in case["roles"].items() if bad[0] in v])


SEEDS = [0, 1, 1 << 32, (1 << 64) - 1]


@pytest.mark.parametrize("shape", [(19, 8, 6), (603, 300, 18)], ids=["n19-group8-A6", "n603-group300-A18"])
def test_seeds_and_offsets(shape):
    """eps = 1 on every row, so every row draws: both halves of the key, and counters whose low word carries inside the
    launch (offset 2^32 - 3) and whose high word is in use (2^40 + 7)"""
    n, group, A = shape
    case = case_of(shape)
    eps = np.ones(n, F)
    seen = set()
    for seed in SEEDS:
        for offset in (0, n, (1 << 32) - 3, (1 << 40) + 7):
            want = R.eps_greedy_ref(case["q"], case["legal"], eps, group, seed, offset)
            assert want["random"].sum() == n - len(case["roles"]["none_legal"])
            got = run_act(case["q"], case["legal"], eps, group, seed, offset)
            assert np.array_equal(got, want["action"]), (seed, offset, np.flatnonzero(got != want["action"])[:8])
            seen.add(got.tobytes())
    assert len(seen) == 16  # (no two of them are the same draws)


@pytest.mark.parametrize("K,A", [(8, 6), (300, 18)])
def test_batching_independence(K, A):
    """'a row's draw does not depend on how rows are batched into launches': 6 K rows in one launch at offset o, and the
    same rows as launches of 2 K and 4 K rows at o and o + 2 K"""
    n = 6 * K
    rng = np.random.default_rng(K)
    q = rng.normal(0, 1, (n, A)).astype(F)
    legal = (rng.uniform(size=(n, A)) < 0.7).astype(F)
    legal[np.arange(n), rng.integers(0, A, n)] = 1
    eps = rng.choice(np.array([0.0, 0.5, 1.0], F), n)
    seed, o = 11, (1 << 32) - K  # (the low counter word carries at the seam of the two launches)
    whole = run_act(q, legal, eps, K, seed, o)
    parts = np.concatenate([run_act(q[:2 * K], legal[:2 * K], eps[:2 * K], K, seed, o),
                            run_act(q[2 * K:], legal[2 * K:], eps[2 * K:], K, seed, o + 2 * K)])
    assert np.array_equal(whole, parts)
    want = R.eps_greedy_ref(q, legal, eps, K, seed, o)
    assert np.array_equal(whole, want["action"]) and 0 < want["random"].sum() < n


# ---- one exact run through each actor ---------------------------------------------------------------------------------------
ACT_R, ACT_K, ACT_A, ACT_N, ACT_TICKS, ACT_SEED, ACT_GAMMA = 16, 8, 6, 2, 6, 11, 0.99
EPS_VALUES = np.array([0.0, 2.0 ** -24, 0.5, 1.0], F)


@functools.lru_cache(maxsize=None)
def actor_inputs():
    """per tick: legal mask [R, A] (changes every tick; row 7 has one legal column), eps [R] from EPS_VALUES (rows 0 and 1:
    always 1; row 2: always 0.5; row 3: 0 and 1 in turn; the rest drawn per tick), rewards"""
    rng = np.random.default_rng(77)
    T, Rr, A = ACT_TICKS, ACT_R, ACT_A
    legal = (rng.uniform(size=(T, Rr, A)) < 0.6).astype(F)
    for t in range(T):
        legal[t, :, t % A] = 1
        legal[t, 7] = 0
        legal[t, 7, (2 * t + 1) % A] = 1
    eps = rng.choice(EPS_VALUES, (T, Rr))
    eps[:, 0] = eps[:, 1] = 1.0
    eps[:, 2] = 0.5
    eps[:, 3] = [0.0, 1.0] * (T // 2)
    rewards = rng.uniform(-1, 1, (T, Rr)).astype(F)
    assert all((legal[t] != legal[t + 1]).any() for t in range(T - 1)) and (eps[1:, 4:] != eps[:-1, 4:]).any()
    assert set(np.unique(eps).tolist()) == set(EPS_VALUES.tolist())
    return legal, eps, rewards


def expected_actions(greedy, legal, eps, seed):
    """action[t][r] = (pick-th legal action of tick t) if u < eps[t][r] else greedy[t][r], u and pick at counter t * R + r"""
    out = [R.eps_select(greedy[t], legal[t], eps[t], seed, R.counters(t * ACT_R, ACT_R)) for t in range(len(greedy))]
    return np.array([o["action"] for o in out]), np.array([o["random"] for o in out])


def check_four_runs(run):
    """run(eps [T, R] or None for all zero, seed) -> actions [T, R].  A: eps = 0 gives the greedy actions (no net's state
    depends on the actions taken, so they are B's too); B: the eps table; then another seed, and B's seed again."""
    legal, eps, _ = actor_inputs()
    greedy = run(None, ACT_SEED)
    b = run(eps, ACT_SEED)
    want, rand = expected_actions(greedy, legal, eps, ACT_SEED)
    assert np.array_equal(b, want), np.argwhere(b != want)[:8]
    # what the comparison rests on: rows went random under 0.5 and stayed greedy under it, and random moved actions
    half = eps == 0.5
    assert rand[half].any() and (~rand[half]).any() and rand[eps == 1.0].all() and not rand[eps < 0.5].any()
    assert (b != greedy)[rand].any() and (legal[np.arange(ACT_TICKS)[:, None], np.arange(ACT_R)[None, :], b] > 0).all()
    other = run(eps, ACT_SEED + 1)
    assert (other != b)[eps == 1.0].any()
    assert np.array_equal(other, expected_actions(greedy, legal, eps, ACT_SEED + 1)[0])
    assert np.array_equal(run(eps, ACT_SEED), b)
    return b


def _apex_run(eps_table, seed, vr_eps=0.0, keep=None):
    """six ticks of an Ape-X shard of 16 rows in groups of 8 -> actions [T, R]; keep (a dict) receives the stored actions
    and obs-side eps of the replay's rows, the priorities of every pop, and the Q tables to restate them from"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.replay import FFReplay
    from synth import synth_obs, synth_params

    Rr, K, A, n, T = ACT_R, ACT_K, ACT_A, ACT_N, ACT_TICKS
    legal, _, rewards = actor_inputs()
    dev = "cuda:0"
    online, target = FFNetHandle(A, dev), FFNetHandle(A, dev)
    online.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 5).items()})
    target.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 6).items()})
    replay = FFReplay(16 * Rr, 3, 0.6, 0.4, 0, A, dev)
    eng = ApexActorEngine(Rr, K, A, n, ACT_GAMMA, replay, np.zeros(Rr, F), dev, seed=seed)
    if vr_eps > 0:
        eng.set_value_rescale(vr_eps)
    nb = capi.lib.rela_ffnet_workspace_bytes(target.h, Rr)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    acts, q_on, q_tg, prios = [], [], [], []
    for t in range(T):
        d_obs = torch.from_numpy(synth_obs(Rr, 100 + t)).to(dev)
        eng.next_obs_slot().copy_(d_obs)
        eng.legal.copy_(torch.from_numpy(legal[t]))
        eng.eps.copy_(torch.from_numpy(eps_table[t] if eps_table is not None else np.zeros(Rr, F)).reshape(Rr, 1))
        acts.append(eng.act(online).cpu().numpy().copy())
        if keep is not None:
            q_on.append(eng.q[0].cpu().numpy().copy())
            d_legal, out = torch.from_numpy(legal[t]).to(dev), torch.empty(Rr, A, device=dev)
            capi.check(capi.lib.rela_ffnet_forward(target.h, Rr, d_obs.data_ptr(), d_legal.data_ptr(), out.data_ptr(),
                                                   ws.data_ptr(), nb, eng._stream()), "rela_ffnet_forward")
            q_tg.append(out.cpu().numpy().copy())
        popped = eng.post_step(torch.from_numpy(rewards[t]).to(dev), torch.zeros(Rr, dtype=torch.uint8, device=dev), online, target)
        assert popped == (t >= n)
        if popped:
            prios.append(eng.prio.cpu().numpy().copy())
    torch.cuda.synchronize()
    if keep is not None:
        rows = (T - n) * Rr
        stored_a, stored_eps = np.zeros(rows, np.int64), np.zeros(rows, F)
        capi.check(capi.lib.rela_replay_debug_read_rows(replay.h, 6, 0, rows, stored_a.ctypes.data_as(C.c_void_p)), "read a")
        capi.check(capi.lib.rela_replay_debug_read_rows(replay.h, 2, 0, rows, stored_eps.ctypes.data_as(C.c_void_p)), "read eps")
        keep.update(stored_a=stored_a.reshape(T - n, Rr), stored_eps=stored_eps.reshape(T - n, Rr), size=replay.size(),
                    prios=np.array(prios), q_on=q_on, q_tg=q_tg)
    eng.close()
    replay.close()
    online.close()
    target.close()
    return np.array(acts)


def _apex_priorities(acts, kept, vr_eps):
    """the priorities of the pops restated from the shard's own Q tables: td_ref in groups of K"""
    from value_rescale_util import nstep_f32

    legal, _, rewards = actor_inputs()
    n = ACT_N
    gamma_n = float(F(float(F(ACT_GAMMA)) ** n))  # (float)pow((double)gamma, n) of the shards
    want = []
    for t in range(n, ACT_TICKS):
        t0 = t - n
        r, b = nstep_f32(rewards[t0:t], np.zeros((n, ACT_R), np.uint8), ACT_GAMMA, n)
        want.append(R.td_ref(kept["q_on"][t0], kept["q_on"][t], kept["q_tg"][t], legal[t], acts[t0], r, b, gamma_n, ACT_K,
                             vr_eps=vr_eps)[1])
    return np.array(want)


def test_apex_actor_draws_at_counter_tick_times_rows_plus_row():
    """... and the transitions that reach the replay carry the action act() returned for their tick and that tick's eps,
    on every row; the priorities of the pops are td_ref's bits in groups of K from the shard's own Q tables, without and
    (the grouped path of that branch) with value rescaling"""
    from value_rescale_util import EPS

    _, eps, _ = actor_inputs()
    kept = {}
    runs = iter([None, kept, None, None])
    b = check_four_runs(lambda e, seed: _apex_run(e, seed, keep=next(runs)))
    n = ACT_N
    assert kept["size"] == (ACT_TICKS - n) * ACT_R
    assert np.array_equal(kept["stored_a"], b[:ACT_TICKS - n])
    assert np.array_equal(kept["stored_eps"], eps[:ACT_TICKS - n]) and (eps[:ACT_TICKS - n] == 1.0).sum() >= 2 * (ACT_TICKS - n)
    assert np.array_equal(kept["prios"].view(np.uint32), _apex_priorities(b, kept, 0.0).view(np.uint32))
    kept_vr = {}
    b_vr = _apex_run(eps, ACT_SEED, vr_eps=EPS, keep=kept_vr)
    assert np.array_equal(b_vr, b)
    want = _apex_priorities(b_vr, kept_vr, EPS)
    assert np.array_equal(kept_vr["prios"].view(np.uint32), want.view(np.uint32))
    assert (kept_vr["prios"] != kept["prios"]).any()


def _r2d2_run(eps_table, seed):
    """six ticks of an R2D2 shard of 16 rows in groups of 8, row 5 terminating at tick 3 -> actions [T, R]"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import LSTMNetHandle, R2D2ActorEngine, dev_view
    from rela_amd.replay import RNNReplay
    from synth import synth_lstm_params, synth_obs

    Rr, K, A, n, T = ACT_R, ACT_K, ACT_A, ACT_N, ACT_TICKS
    seq, burn = 4, 2
    legal, _, rewards = actor_inputs()
    dev = "cuda:0"
    online, target = LSTMNetHandle(A, dev), LSTMNetHandle(A, dev)
    online.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, 1).items()})
    target.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, 2).items()})
    replay = RNNReplay(64, 7, 0.6, 0.4, 0, A, burn + seq + n, dev)
    eng = R2D2ActorEngine(Rr, K, A, n, 0.997, seq, burn, 0.9, replay, np.zeros(Rr, F), dev, seed=seed)
    acts = []
    for t in range(T):
        eng.next_obs_slot().copy_(torch.from_numpy(synth_obs(Rr, 300 + t)).to(dev))
        e = np.ascontiguousarray(eps_table[t] if eps_table is not None else np.zeros(Rr, F), F)
        lg = np.ascontiguousarray(legal[t])
        out = C.c_void_p()  # this tick's own eps and legal mask go in with the call
        capi.check(capi.lib.rela_r2d2_actor_act(eng.h, online.h, None, e.ctypes.data_as(C.c_void_p), lg.ctypes.data_as(C.c_void_p),
                                                None, C.byref(out), eng._stream()), "rela_r2d2_actor_act")
        acts.append(dev_view(out.value, (Rr,), torch.int64, eng.device).cpu().numpy().copy())
        term = np.zeros(Rr, np.uint8)
        term[5] = t == 3
        eng.post_step(np.ascontiguousarray(rewards[t]), term, online, target)
    torch.cuda.synchronize()
    eng.close()
    replay.close()
    online.close()
    target.close()
    return np.array(acts)


def test_r2d2_actor_draws_at_counter_tick_times_rows_plus_row():
    check_four_runs(_r2d2_run)
