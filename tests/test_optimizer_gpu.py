"""The step of both learners that turns gradients into weights, one call at a time (include/rela_amd.h, csrc/learner_common.hip):
  rela_debug_optimizer_apply     optimizer_apply: sumsq_partial, clip_coef, rmsprop_update / adam_update
against tests/optim_ref.py: the float32 restatement in the kernels' order BIT FOR BIT, the float64 form within the bound counted
from the roundings, on tables by role:
  a. sentinel norms at every length where sumsq_partial takes another path: an exact sum, so a dropped or doubled element
     changes known digits of the norm; the weights of zero-gradient elements come back unchanged;
  b. dense tables (gradients over sixteen decades, zeros, squares that are denormal or underflow) from a zero state and from
     the state of a previous apply, with the test's and the workloads' hyper-parameters;
  c. the clip regimes: coefficient exactly 1, norm == clip, norm = 1000 * clip, all-zero gradients;
  d. 12 applies carrying state; Adam 0, 1, 9, 10^4 and 10^6 steps in;
  e. the skip path (abort word), NaN and inf gradients, bad arguments;
  f. the learners run this code: apply() of both learners with both optimisers equals the tap on copies, state and step number
     included; the pad floats of the flat buffers stay zero; a skipped apply costs no Adam step number.
tests/test_optim_ref_cpu.py pins the references and shows which restated defects these tables catch."""
import ctypes as C

import numpy as np
import pytest

import optim_ref as R

pytestmark = pytest.mark.gpu

OPTS = ("rmsprop", "adam")
HP = R.hp32(R.TEST_HP)
CENSUS = {opt: {"sumsq_partial": 1, "clip_coef": 1, "%s_update" % opt: 1} for opt in OPTS}
KEYS = ("p", "s1", "s2", "norm", "coef")
GUARD = 2.0 ** 60


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def tap(opt, p, g, s1, s2, stats, t, hp, abort=0):
    """rela_debug_optimizer_apply on device tensors, in place.  -> (skip counter, census)"""
    from rela_amd import _capi as capi

    skipped = C.c_uint(12345)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_optimizer_apply(
            OPTS.index(opt), hp["lr"], hp["eps"], hp["clip"], t, p.numel(), ptr(p), ptr(g), ptr(s1), ptr(s2), ptr(stats), abort,
            C.byref(skipped), _stream()), "rela_debug_optimizer_apply")
    return skipped.value, census.counts


def apply(opt, p, g, s1, s2, t, hp, abort=0):
    """one apply of numpy float32 arrays on the device.  -> dict(p, s1, s2, norm, coef, skipped) of numpy values"""
    import torch

    # every buffer sits in front of one guard float4 of 2^60: a gradient read past the end shows in the norm (the unrolled
    # loop of sumsq_partial with `<=` for `<` reads exactly that float4 at 3 * 65,536 float4), a write past the end in the guard
    n = np.asarray(p).size
    room = [torch.full((n + 4,), GUARD, dtype=torch.float32, device="cuda") for _ in range(4)]
    dev = [r[:n] for r in room]
    for d, x in zip(dev, (p, g, s1, s2)):
        d.copy_(torch.from_numpy(np.array(x, dtype=np.float32)))
    stats = torch.full((2,), float("nan"), device="cuda")
    skipped, counts = tap(opt, dev[0], dev[1], dev[2], dev[3], stats, t, hp, abort)
    assert counts == CENSUS[opt], counts
    assert np.array_equal(dev[1].cpu().numpy().view(np.int32), np.asarray(g, dtype=np.float32).view(np.int32))  # g is read only
    for r in room:
        assert bool((r[n:] == GUARD).all()), "a kernel wrote past the end of a buffer"
    st = stats.cpu().numpy()
    return dict(p=dev[0].cpu().numpy(), s1=dev[2].cpu().numpy(), s2=dev[3].cpu().numpy(), norm=st[0], coef=st[1],
                skipped=skipped)


def assert_bits(got, want, what, keys=KEYS):
    for k in keys:
        if not R.same_bits(got[k], want[k]):
            u = np.atleast_1d(R.ulps(got[k], want[k]))
            i = int(np.nanargmax(u))
            raise AssertionError("%s: %s differs from the float32 form in %d of %d elements; worst at %d: got %r, expected %r "
                                 "(%.3g ulps)" % (what, k, int(np.count_nonzero(u)), u.size, i, np.atleast_1d(got[k])[i],
                                                  np.atleast_1d(want[k])[i], u[i]))


def assert_within_f64(opt, got, p, g, s1, s2, t, hp, what, record=None):
    """against the float64 form with the kernels' constants from the same inputs, within f32_bound"""
    ref = R.step_f64(opt, p, g, s1, s2, t, hp["lr"], hp["eps"], hp["clip"], R.KERNEL_CONSTS)
    a_abs = R.KERNEL_CONSTS["b1"] * np.abs(np.asarray(s1, dtype=np.float64)) + R.KERNEL_CONSTS["one_m_b1"] * np.abs(
        np.asarray(g, dtype=np.float64) * ref["coef"])
    zero = not np.any(s1) and not np.any(s2)
    bound = R.f32_bound(opt, ref, a_abs, R.sq_avg_roundings(0, zero), R.adam_a_roundings(0, zero), t + 1, hp["lr"], hp["eps"])
    for k in KEYS:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        units = float(np.max(err / np.maximum(bound[k], 1e-300)))
        print("%s: %s at %.3g of its float64 bound" % (what, k, units))
        if record:
            record("f64_units_%s" % k, units)
        assert units <= 1.0, (what, k, units)


def zeros(n):
    return np.zeros(n, dtype=np.float32)


def uniform_params(n, seed):
    return np.random.default_rng([seed, 5]).uniform(-1, 1, n).astype(np.float32)


# ---- a. sentinel norms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n4", R.LENGTHS4)
def test_sentinel_norm_counts_every_element_once(n4):
    """26 sentinels +-2^k at the edges of sumsq_partial's loops (fewer where the buffer is shorter), rotated three times so
    that every edge holds a sentinel the float32 norm shows: the sum of squares is exact in float64 whatever the order, so
    stats[0] IS float32(sqrt(exact)).  Everything else of the apply equals the float32 form, and a zero gradient leaves
    its weight alone (Adam: from a zero state)."""
    n = 4 * n4
    p = uniform_params(n, n4)
    for rot in R.SENTINEL_ROTATIONS:
        g, total, pos = R.sentinel_grads(n4, rot)
        for opt in OPTS:
            got = apply(opt, p, g, zeros(n), zeros(n), 0, HP)
            assert R.same_bits(got["norm"], R.sentinel_norm(total)), (rot, opt, got["norm"], R.sentinel_norm(total))
            assert_bits(got, R.step_f32(opt, p, g, zeros(n), zeros(n), 0, **HP), "n4 %d rot %d %s" % (n4, rot, opt))
            still = g == 0
            assert R.same_bits(got["p"][still], p[still]) and not got["s1"][still].any() and not got["s2"][still].any()
            assert bool((got["p"][~still] != p[~still]).all())


# ---- b. dense tables -----------------------------------------------------------------------------------------------------------
DENSE = [(n4, R.TEST_HP) for n4 in R.LENGTHS4] + [(n4, R.WORKLOAD_HP) for n4 in (257, 65537, 7 * 65536 + 5)]


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("n4,hp", DENSE, ids=["n4_%d-lr%g" % (n4, hp["lr"]) for n4, hp in DENSE])
def test_dense_tables_bit_for_bit(n4, hp, opt, record_property):
    """one apply from a zero state, a second one from the first one's state with fresh gradients: p, s1, s2, norm and
    coefficient equal the float32 form bit for bit and lie within the derived bound of the float64 form"""
    n, seed, hp = 4 * n4, R.dense_seed(n4), R.hp32(hp)
    g = R.dense_grads(n, seed)
    p, s1, s2 = R.dense_params(opt, g, zeros(n), zeros(n), 0, hp["lr"], hp["eps"], hp["clip"], seed), zeros(n), zeros(n)
    for k in range(2):
        g = R.dense_grads(n, seed, k)
        got = apply(opt, p, g, s1, s2, k, hp)
        what = "n4 %d %s apply %d" % (n4, opt, k)
        assert_bits(got, R.step_f32(opt, p, g, s1, s2, k, **hp), what)
        assert_within_f64(opt, got, p, g, s1, s2, k, hp, what, record_property if k == 1 else None)
        moved = R.moved_ulps(p, got["p"])[g != 0]
        assert moved.size == 0 or float(moved.min()) >= 8, (what, float(moved.min()))  # the table shows every step
        p, s1, s2 = got["p"], got["s1"], got["s2"]


# ---- c. clip regimes -----------------------------------------------------------------------------------------------------------
N4_REGIME = 65537


@pytest.mark.parametrize("opt", OPTS)
def test_clip_regimes(opt):
    import torch

    n = 4 * N4_REGIME
    z = zeros(n)
    g = R.dense_grads(n, 9)
    p = R.dense_params(opt, g, z, z, 0, HP["lr"], HP["eps"], HP["clip"], 9)
    # norm far below clip: the coefficient is exactly 1, and the clip value takes no further part
    small = (g * np.float32(2.0 ** -30)).astype(np.float32)
    got = apply(opt, p, small, z, z, 0, HP)
    wide = apply(opt, p, small, z, z, 0, dict(HP, clip=1e30))
    assert float(got["norm"]) < 1e-2 * HP["clip"] and got["coef"] == 1.0 and wide["coef"] == 1.0
    assert_bits(got, wide, "%s unclipped against clip 1e30" % opt)
    assert_bits(got, R.step_f32(opt, p, small, z, z, 0, **HP), "%s unclipped" % opt)
    # norm == clip exactly (0.375, 0.5 -> 0.625): the coefficient is the float below 1 that clip / (norm + 1e-6f) gives
    eq = zeros(n)
    eq[5], eq[n - 2] = 0.375, -0.5
    hp = dict(HP, clip=0.625)
    got = apply(opt, p, eq, z, z, 0, hp)
    c = np.float32(0.625) / (np.float32(0.625) + np.float32(1e-6))
    assert got["norm"] == np.float32(0.625) and R.same_bits(got["coef"], c) and c < 1 and c > np.float32(0.99999)
    assert_bits(got, R.step_f32(opt, p, eq, z, z, 0, **hp), "%s norm == clip" % opt)
    # norm = 1000 * clip
    norm = float(R.clip_f32(g, 1.0)[0])
    hp = dict(HP, clip=float(np.float32(norm / 1000)))
    got = apply(opt, p, g, z, z, 0, hp)
    assert abs(float(got["coef"]) - 1e-3) < 1e-8
    assert_bits(got, R.step_f32(opt, p, g, z, z, 0, **hp), "%s norm 1000 clip" % opt)
    prev = got
    # all-zero gradients: the coefficient is 1; from a zero state nothing moves; a previous state decays as restated,
    # and RMSprop still leaves p alone
    got = apply(opt, p, z, z, z, 0, HP)
    assert got["norm"] == 0 and got["coef"] == 1.0 and R.same_bits(got["p"], p) and not got["s1"].any() and not got["s2"].any()
    got = apply(opt, prev["p"], z, prev["s1"], prev["s2"], 1, HP)
    assert got["norm"] == 0 and got["coef"] == 1.0
    assert_bits(got, R.step_f32(opt, prev["p"], z, prev["s1"], prev["s2"], 1, **HP), "%s zero gradients" % opt)
    if opt == "rmsprop":
        assert R.same_bits(got["p"], prev["p"]) and R.same_bits(got["s1"], np.float32(0.99) * prev["s1"])
    else:
        assert R.same_bits(got["s1"], np.float32(0.9) * prev["s1"]) and R.same_bits(got["s2"], np.float32(0.999) * prev["s2"])
    torch.cuda.synchronize()


# ---- d. steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTS)
def test_twelve_applies_carrying_state(opt):
    """the device's own buffers carried over 12 applies against the float32 form carried alongside"""
    import torch

    n4 = 65537
    n, seed = 4 * n4, 21
    g = R.dense_grads(n, seed)
    p = R.dense_params(opt, g, zeros(n), zeros(n), 0, HP["lr"], HP["eps"], HP["clip"], seed)
    ref = dict(p=p, s1=zeros(n), s2=zeros(n))
    dp, ds1, ds2 = (torch.from_numpy(ref[k].copy()).cuda() for k in ("p", "s1", "s2"))
    stats = torch.zeros(2, device="cuda")
    for k in range(12):
        g = R.dense_grads(n, seed, k)
        skipped, counts = tap(opt, dp, torch.from_numpy(g).cuda(), ds1, ds2, stats, k, HP)
        assert skipped == 0 and counts == CENSUS[opt]
        ref = R.step_f32(opt, ref["p"], g, ref["s1"], ref["s2"], k, **HP)
        st = stats.cpu().numpy()
        got = dict(p=dp.cpu().numpy(), s1=ds1.cpu().numpy(), s2=ds2.cpu().numpy(), norm=st[0], coef=st[1])
        assert_bits(got, ref, "%s apply %d" % (opt, k))


@pytest.mark.parametrize("t", R.ADAM_STEPS_DONE)
def test_adam_steps_done(t, record_property):
    """the host's bias corrections (pow and sqrt in double, cast to float) 0, 1, 9, 10^4 and 10^6 steps in; at the last
    0.9^t has underflowed and bc1 is exactly 1.0f"""
    n4 = 257
    n, seed = 4 * n4, 30
    g0 = R.dense_grads(n, seed)
    p0 = R.dense_params("adam", g0, zeros(n), zeros(n), t, HP["lr"], HP["eps"], HP["clip"], seed)
    first = apply("adam", p0, g0, zeros(n), zeros(n), t, HP)
    assert_bits(first, R.step_f32("adam", p0, g0, zeros(n), zeros(n), t, **HP), "t %d" % t)
    g1 = R.dense_grads(n, seed, 1)
    got = apply("adam", first["p"], g1, first["s1"], first["s2"], t + 1, HP)
    assert_bits(got, R.step_f32("adam", first["p"], g1, first["s1"], first["s2"], t + 1, **HP), "t %d + 1" % t)
    assert_within_f64("adam", got, first["p"], g1, first["s1"], first["s2"], t + 1, HP, "t %d + 1" % t, record_property)
    if t == 10 ** 6:
        assert R.bias_corrections_f32(t + 1)[0] == np.float32(1.0)
    else:  # the step number matters: one more or one less changes the weights
        other = apply("adam", p0, g0, zeros(n), zeros(n), t + 1, HP)
        assert not R.same_bits(other["p"], first["p"])


# ---- e. skip, non-finite, arguments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTS)
def test_abort_word_skips_the_update_and_counts_it(opt):
    n4 = 257
    n, seed = 4 * n4, 40
    g = R.dense_grads(n, seed)
    p = R.dense_params(opt, g, zeros(n), zeros(n), 0, HP["lr"], HP["eps"], HP["clip"], seed)
    first = apply(opt, p, g, zeros(n), zeros(n), 0, HP)
    assert first["skipped"] == 0
    g1 = R.dense_grads(n, seed, 1)
    got = apply(opt, first["p"], g1, first["s1"], first["s2"], 1, HP, abort=1)
    assert got["coef"] == -1.0 and got["skipped"] == 1
    assert R.same_bits(got["norm"], R.clip_f32(g1, HP["clip"])[0])  # the norm is still the norm
    for k in ("p", "s1", "s2"):
        assert R.same_bits(got[k], first[k]), k
    # a following normal apply with the same number of steps done: as if the skipped one had never been
    after = apply(opt, got["p"], g1, got["s1"], got["s2"], 1, HP)
    assert_bits(after, R.step_f32(opt, first["p"], g1, first["s1"], first["s2"], 1, **HP), "%s after a skip" % opt)
    assert after["skipped"] == 0


@pytest.mark.parametrize("opt", OPTS)
def test_nan_and_inf_gradients(opt):
    """torch's clip_grad_norm_: a NaN gradient makes the coefficient and so every weight NaN; an inf gradient gives (inf, 0),
    NaN in its own weight, and moves the others as a zero gradient does"""
    n4 = 65537  # more than one visit
    n, seed, at = 4 * n4, 50, 4 * 65536 + 2
    g0 = R.dense_grads(n, seed)
    p = R.dense_params(opt, g0, zeros(n), zeros(n), 0, HP["lr"], HP["eps"], HP["clip"], seed)
    prev = apply(opt, p, g0, zeros(n), zeros(n), 0, HP)
    g = R.dense_grads(n, seed, 1)
    g[at] = np.nan
    got = apply(opt, prev["p"], g, prev["s1"], prev["s2"], 1, HP)
    assert np.isnan(got["norm"]) and np.isnan(got["coef"]) and np.isnan(got["p"]).all()
    others = np.arange(n) != at
    for bad in (np.inf, -np.inf):
        g[at] = bad
        got = apply(opt, prev["p"], g, prev["s1"], prev["s2"], 1, HP)
        zero_g = apply(opt, prev["p"], zeros(n), prev["s1"], prev["s2"], 1, HP)
        assert got["norm"] == np.inf and got["coef"] == 0.0 and np.isnan(got["p"][at])
        for k in ("p", "s1", "s2"):
            assert R.same_bits(got[k][others], zero_g[k][others]), (bad, k)
        assert_bits(got, R.step_f32(opt, prev["p"], g, prev["s1"], prev["s2"], 1, **HP), "%s inf" % opt)


def test_bad_arguments_are_refused():
    import torch

    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    lib = capi.lib
    buf = [torch.zeros(64, device="cuda") for _ in range(5)]
    p = [ptr(b) for b in buf]

    def args(optimizer=0, t=0, n=32, ptrs=p, abort=0):
        return [optimizer, 1e-3, 1.5e-4, 40.0, t, n] + list(ptrs) + [abort, None, None]

    assert lib.rela_debug_optimizer_apply(*args()) == capi.OK  # (the refusals below are refusals of their argument)
    assert lib.rela_debug_optimizer_apply(*args(optimizer=1)) == capi.OK
    for kw in ({"n": 0}, {"n": -4}, {"n": 30}, {"n": 33}, {"optimizer": 2}, {"optimizer": -1}, {"t": -1}, {"abort": 2}):
        assert lib.rela_debug_optimizer_apply(*args(**kw)) == capi.EINVAL, kw
    for hole in range(5):
        ptrs = list(p)
        ptrs[hole] = None
        assert lib.rela_debug_optimizer_apply(*args(ptrs=ptrs)) == capi.EINVAL, hole
    for bent in range(4):  # p, g, s1, s2 off their 16 bytes
        ptrs = list(p)
        ptrs[bent] = C.c_void_p(buf[bent].data_ptr() + 4)
        assert lib.rela_debug_optimizer_apply(*args(ptrs=ptrs)) == capi.EINVAL, bent
    assert b"aligned" in lib.rela_last_error()
    assert not any(bool(b.any()) for b in (buf[0], buf[2], buf[3]))  # (all-zero gradients: nothing moved either way)

    out = [C.c_void_p(), C.c_void_p()]
    t = C.c_int64()
    for name, learner in (("rela_apex_learner_debug_optim", HipApexLearner(6, 4, 2, 0.99)),
                          ("rela_r2d2_learner_debug_optim", HipR2D2Learner(6, 4, 2, 0.997, 7, 0, 0.9))):
        fn = getattr(lib, name)
        assert fn(None, C.byref(out[0]), C.byref(out[1]), C.byref(t)) == capi.EINVAL
        assert fn(learner.h, None, C.byref(out[1]), C.byref(t)) == capi.EINVAL
        assert fn(learner.h, C.byref(out[0]), C.byref(out[1]), None) == capi.EINVAL
        assert fn(learner.h, C.byref(out[0]), C.byref(out[1]), C.byref(t)) == capi.OK and out[0].value and out[1].value
        learner.close()
    assert lib.rela_r2d2_learner_debug_set_timeout_word(None, 1, None) == capi.EINVAL
    torch.cuda.synchronize()


# ---- f. through the learners ---------------------------------------------------------------------------------------------------
A = 6
WORKLOAD = R.hp32(R.WORKLOAD_HP)


def make_learner(algo, opt, hp=WORKLOAD, max_batch=4):
    """a learner with synthetic weights -> (learner, [(key, shape, offset)], total)"""
    import torch

    from rela_amd.learner import HipApexLearner, HipR2D2Learner, ffnet_flat_layout, lstmnet_flat_layout
    from synth import synth_lstm_params, synth_params

    kw = dict(optimizer=opt, lr=hp["lr"], eps=hp["eps"], grad_clip=hp["clip"])
    if algo == "apex":
        learner, params, (layout, total) = HipApexLearner(A, max_batch, 3, 0.99, **kw), synth_params(A, 61), ffnet_flat_layout(A)
    else:
        learner = HipR2D2Learner(A, max_batch, 2, 0.997, 7, 0, 0.9, **kw)
        params, (layout, total) = synth_lstm_params(A, 62), lstmnet_flat_layout(A)
    learner.load_state_dicts({k: torch.from_numpy(v).cuda() for k, v in params.items()})
    return learner, layout, total


def pad_mask(layout, total):
    """True at the floats of the flat buffer that belong to no tensor"""
    mask = np.ones(total, dtype=bool)
    for _, shape, off in layout:
        mask[off:off + int(np.prod(shape))] = False
    return mask


def table_gradients(total, pads, seed, step):
    import torch

    g = R.dense_grads(total, seed, step)
    g[pads] = 0
    return torch.from_numpy(g).cuda()


def bits(t):
    import torch

    return t.detach().contiguous().view(torch.int32)


LEARNERS = [("apex", "rmsprop"), ("apex", "adam"), ("r2d2", "adam"), ("r2d2", "rmsprop")]


@pytest.mark.parametrize("algo,opt", LEARNERS)
def test_apply_of_the_learners_is_the_tap(algo, opt):
    """three apply() calls on dense gradient tables written into the learner's flat gradient buffer (pads zero): parameters,
    both state buffers, stats and the Adam step number equal three tap calls on copies, bit for bit"""
    import torch

    learner, layout, total = make_learner(algo, opt)
    pads = pad_mask(layout, total)
    assert pads.any() and total % 4 == 0
    P, G = learner.flat()
    S1, S2, t = learner.debug_optim()
    assert P.numel() == G.numel() == S1.numel() == S2.numel() == total and t == 0
    assert not bool(S1.any()) and not bool(S2.any())
    tp, ts1, ts2, stats = P.clone(), S1.clone(), S2.clone(), torch.zeros(2, device="cuda")
    for k in range(3):
        g = table_gradients(total, pads, 70, k)
        G.copy_(g)
        learner.apply()
        skipped, counts = tap(opt, tp, g, ts1, ts2, stats, k, WORKLOAD)
        torch.cuda.synchronize()
        assert skipped == 0 and counts == CENSUS[opt]
        for name, own, mine in (("P", P, tp), ("S1", S1, ts1), ("S2", S2, ts2), ("stats", learner.stats(), stats)):
            assert torch.equal(bits(own), bits(mine)), (k, name)
        assert float(stats[1]) < 1 and bool((tp != 0).any())
        assert learner.debug_optim()[2] == (k + 1 if opt == "adam" else 0)
        sd = learner.state_dict("online")  # the views sit in P
        assert torch.equal(sd[layout[-1][0]].reshape(-1), P[layout[-1][2]:layout[-1][2] + A])
    if opt == "rmsprop":
        assert not bool(S2.any())
    learner.close()


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_pad_floats_stay_zero_through_a_real_step(algo):
    """one real backward at the smallest batch of the learners' own tests: the pads of G are exactly zero, stats()[0] is
    the norm over the tensors' own elements, and apply() leaves the pads of P, S1 and S2 exactly zero"""
    import torch

    from rela_amd.learner import HipApexLearner, HipR2D2Learner, ffnet_flat_layout, lstmnet_flat_layout

    # (the helpers draw from torch's global generators: forked, so that the tests after this one see the stream they
    # would see without it)
    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(6005)
        if algo == "apex":
            from test_learner_gpu import make_agent, make_batch

            B = 32
            learner = HipApexLearner.from_agent(make_agent(A, 5), B, optimizer="adam")
            batch, w = make_batch(B, A, 4)
            layout, total = ffnet_flat_layout(A)
        else:
            from test_r2d2_learner_gpu import _agent, _random_batch

            B, seq, burn, n = 5, 7, 0, 2
            learner = HipR2D2Learner.from_agent(_agent(A, n, 0.997, 0.9, seq, burn, 71, 72, "cuda:0"), B)
            batch, w = _random_batch(np.random.default_rng(6005), A, B, seq, burn, n, "cuda:0")
            layout, total = lstmnet_flat_layout(A)
    pads = torch.from_numpy(pad_mask(layout, total)).cuda()
    P, G = learner.flat()
    assert int(pads.sum()) > 0 and not bool(P[pads].any()) and not bool(G[pads].any())
    learner.backward(batch, w)
    if algo == "r2d2":
        learner.check()
    torch.cuda.synchronize()
    assert not bool(G[pads].any()), "a backward kernel wrote into the pad floats of G"
    grads = learner.state_dict("grads")
    own = sum(float((v.double() ** 2).sum()) for v in grads.values())
    assert own > 0 and abs(own - float((G.double() ** 2).sum())) <= 1e-12 * own
    learner.apply()
    torch.cuda.synchronize()
    assert float(learner.stats()[0]) == float(np.float32(np.sqrt(own)))
    S1, S2, t = learner.debug_optim()
    assert t == 1 and bool(S1.any()) and bool(S2.any())
    for name, buf in (("P", P), ("S1", S1), ("S2", S2)):
        assert not bool(buf[pads].any()), name
    learner.close()


def test_a_skipped_apply_costs_no_adam_step_number():
    """R2D2, Adam: two applies, the timeout word set (a stream-ordered store: nothing times out), two applies that the device
    skips, check(), one apply.  While the word is set only apply() and check() run.  Weights and state after the skipped
    applies are the ones before them; check() reports RELA_ESTATE and takes the two skipped applies off the step number; the
    last apply equals the tap with two steps done."""
    import torch

    from rela_amd import _capi as capi

    learner, layout, total = make_learner("r2d2", "adam")
    pads = pad_mask(layout, total)
    P, G = learner.flat()
    S1, S2, _ = learner.debug_optim()
    stream = _stream()
    for k in range(2):
        G.copy_(table_gradients(total, pads, 80, k))
        learner.apply()
    learner.check()  # nothing to report
    before = [x.clone() for x in (P, S1, S2)]
    assert learner.debug_optim()[2] == 2
    capi.check(capi.lib.rela_r2d2_learner_debug_set_timeout_word(learner.h, 7, stream), "set_timeout_word")
    for k in (2, 3):
        G.copy_(table_gradients(total, pads, 80, k))
        norm = float(np.float32(R.clip_f32(G.cpu().numpy(), WORKLOAD["clip"])[0]))
        learner.apply()
        torch.cuda.synchronize()
        st = learner.stats().cpu().numpy()
        assert st[1] == -1.0 and float(st[0]) == norm
        for own, kept in zip((P, S1, S2), before):
            assert torch.equal(bits(own), bits(kept)), k
    assert learner.debug_optim()[2] == 4  # the host counted both before it could know
    assert capi.lib.rela_r2d2_learner_check(learner.h, stream) == capi.ESTATE
    assert b"timed out at step 6" in capi.lib.rela_last_error()
    assert learner.debug_optim()[2] == 2
    assert capi.lib.rela_r2d2_learner_check(learner.h, stream) == capi.OK  # word and counter are cleared
    assert learner.debug_optim()[2] == 2
    g = table_gradients(total, pads, 80, 4)
    G.copy_(g)
    learner.apply()
    stats = torch.zeros(2, device="cuda")
    skipped, _ = tap("adam", before[0], g, before[1], before[2], stats, 2, WORKLOAD)
    torch.cuda.synchronize()
    assert skipped == 0 and learner.debug_optim()[2] == 3
    for name, own, mine in (("P", P, before[0]), ("S1", S1, before[1]), ("S2", S2, before[2]), ("stats", learner.stats(), stats)):
        assert torch.equal(bits(own), bits(mine)), name
    assert float(stats[1]) > 0
    learner.close()
