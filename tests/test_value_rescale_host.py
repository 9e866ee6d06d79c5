"""Invertible value rescaling h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x, CPU side.

  1. rela_amd/csrc/value_rescale.h compiled for the host (tests/cpu_shims/value_rescale_host.cpp) against a float64
     numpy evaluation of the textbook formulas on a grid that covers the cancelling regions: h, h_inv and the round trip
     h_inv(h(x)).  The bound is relative to the float32 torch textbook form pyrela uses: the header must be at least as
     accurate as that form on the same inputs.
  2. ApexAgent / R2D2Agent with value_rescale=1e-3 against a float64 closed-form restatement of the target written here,
     and with value_rescale=0 bit-equal to an agent constructed without the argument.
"""
import numpy as np

from value_rescale_util import (EPS, apex_agent, grid, h64, hinv64, host_h_hinv, max_err, r2d2_agent, scale_rewards,
                                torch_textbook)

# every intermediate of the header's two functions is one correctly rounded float32 operation on positive terms; h has
# six of them (a + 1, sqrt, s + 1, the quotient, eps x, the sum), h_inv nine, and sqrt halves the error of its argument:
# the result is within 8 * 2^-24 = 4.8e-7 of the exact value, relative
HEADER_REL_BOUND = 8 * 2.0 ** -24


def test_header_is_at_least_as_accurate_as_the_float32_textbook_form(record_property):
    x = grid()
    assert x.size > 8000 and (x == 0).sum() == 1
    h, hi = host_h_hinv(x)
    th, thi = torch_textbook(x)
    ref_h, ref_hi = h64(x), hinv64(x)
    err = {"h_header": max_err(h, ref_h), "h_textbook_f32": max_err(th, ref_h), "hinv_header": max_err(hi, ref_hi),
           "hinv_textbook_f32": max_err(thi, ref_hi)}
    for k, v in err.items():
        record_property("max_rel_err_" + k, v)
    print("max relative error against float64: " + ", ".join("%s %.3g" % kv for kv in err.items()))
    assert err["h_header"] <= err["h_textbook_f32"], err
    assert err["hinv_header"] <= err["hinv_textbook_f32"], err
    assert err["h_header"] <= HEADER_REL_BOUND and err["hinv_header"] <= HEADER_REL_BOUND, err
    # signs, and the point where the true value is 0
    assert h[0] == 0 and hi[0] == 0
    assert np.array_equal(np.sign(h), np.sign(x)) and np.array_equal(np.sign(hi), np.sign(x))


def test_round_trip_is_at_least_as_accurate_as_the_float32_textbook_form(record_property):
    x = grid()
    h, _ = host_h_hinv(x)
    _, back = host_h_hinv(h)
    th, _ = torch_textbook(x)
    _, tback = torch_textbook(th)
    # = x up to the float64 rounding of the textbook inverse, whose cancelling sqrt(1 + z) - 1 is divided by 2 eps: a few
    # 2^-53 / 2e-3 = 1e-13 absolute, which is also what this reference can resolve at the smallest |x| of the grid
    ref = hinv64(h64(x))
    assert np.all(np.abs(ref - x) <= 1e-12 * (1.0 + np.abs(x)))
    e_hdr, e_txt = max_err(back, ref), max_err(tback, ref)
    record_property("max_rel_err_round_trip_header", e_hdr)
    record_property("max_rel_err_round_trip_textbook_f32", e_txt)
    print("round trip h_inv(h(x)): header %.3g, float32 textbook %.3g" % (e_hdr, e_txt))
    assert e_hdr <= e_txt, (e_hdr, e_txt)
    # h_inv amplifies the rounding of h(x) by at most (h / x) / h'(x) < 2 (reached as |x| grows): 2 * bound + bound
    assert e_hdr <= 3 * HEADER_REL_BOUND, e_hdr


def test_another_eps():
    """eps is a parameter of the header: the same accuracy at 1e-2.  (A smaller eps is not checked this way: the float64
    textbook inverse divides its own cancellation error by 2 eps and stops resolving the header's error at small |x|.)"""
    x = grid()
    eps = float(np.float32(1e-2))
    h, hi = host_h_hinv(x, eps)
    assert max_err(h, h64(x, eps)) <= HEADER_REL_BOUND
    assert max_err(hi, hinv64(x, eps)) <= HEADER_REL_BOUND


# ---- agent modules ---------------------------------------------------------------------------------------------
# The float32 textbook h_inv carries the rounding of sqrt(1 + z) near 1 divided by 2 eps: (2^-24 + 2^-25) / 2e-3 = 4.5e-5
# in u, times (u + 1) ~ 2 in u^2 - 1: 9e-5 in the bootstrap value; h'(x) <= 0.5 + eps halves it, and the float32
# roundings of values up to h(1e3 + ...) ~ 32 add a few 2e-6.  Twice that:
AGENT_ATOL = 2e-4


def _apex_batch(B, A, seed):
    from test_learner_gpu import make_batch

    batch, w = make_batch(B, A, seed, device="cpu")
    return scale_rewards(batch, np.random.default_rng(seed)), w


def test_apex_agent_matches_the_closed_form_and_off_is_bit_equal():
    import torch

    A, B = 6, 8
    batch, _ = _apex_batch(B, A, 5)
    assert float(batch.reward.abs().max()) > 100
    on = apex_agent(A, 3, 1e-3)
    err = on.td_err(batch.obs, batch.action, batch.reward, batch.bootstrap, batch.next_obs)
    with torch.no_grad():
        q = on.online_net(batch.obs).double().numpy()
        qn = on.online_net(batch.next_obs).numpy()
        qt = on.target_net(batch.next_obs).double().numpy()
    nl = batch.next_obs["legal_move"].numpy()
    na = ((1 + qn - qn.min()) * nl).argmax(1)
    rows = np.arange(B)
    r, b = batch.reward.double().numpy(), batch.bootstrap.double().numpy()
    target = h64(r + b * (0.99 ** 3) * hinv64(qt[rows, na], 1e-3), 1e-3)
    ref = target - q[rows, batch.action["a"].numpy()]
    plain = r + b * (0.99 ** 3) * qt[rows, na] - q[rows, batch.action["a"].numpy()]
    assert np.abs(ref - plain).max() > 10  # the rescaling matters on these inputs
    np.testing.assert_allclose(err.detach().numpy(), ref, rtol=0, atol=AGENT_ATOL)
    per_sample, prio = on.loss(batch)
    ref_loss = np.where(np.abs(ref) < 1, 0.5 * ref * ref, np.abs(ref) - 0.5)
    np.testing.assert_allclose(per_sample.detach().numpy(), ref_loss, rtol=0, atol=AGENT_ATOL)
    np.testing.assert_allclose(prio.numpy(), np.abs(ref), rtol=0, atol=AGENT_ATOL)
    pr = on.compute_priority(batch.obs, batch.action, batch.reward, batch.terminal, batch.bootstrap, batch.next_obs)
    np.testing.assert_allclose(pr.numpy(), np.abs(ref), rtol=0, atol=AGENT_ATOL)
    twin = type(on).clone(on, "cpu")
    assert twin.value_rescale == on.value_rescale
    assert torch.equal(twin.td_err(batch.obs, batch.action, batch.reward, batch.bootstrap, batch.next_obs), err)
    # off: bit-equal to an agent that never heard of the argument
    zero, bare = apex_agent(A, 3, 0.0), apex_agent(A, 3, None)
    assert bare.value_rescale == 0.0
    for a, b_ in zip(zero.loss(batch), bare.loss(batch)):
        assert torch.equal(a, b_)
    np.testing.assert_allclose(
        bare.td_err(batch.obs, batch.action, batch.reward, batch.bootstrap, batch.next_obs).detach().numpy(), plain,
        rtol=0, atol=AGENT_ATOL)


def _r2d2_batch(A, B, seq, burn, n, seed):
    from test_r2d2_learner_gpu import _random_batch

    for s in range(seed, seed + 64):  # the first seed whose batch has a padded sequence next to a full one
        rng = np.random.default_rng(s)
        batch, w = _random_batch(rng, A, B, seq, burn, n, "cpu")
        if float(batch.seq_len.min()) < burn + seq:
            return scale_rewards(batch, rng), w
    raise AssertionError("no padded sequence")


def test_r2d2_agent_matches_the_closed_form_and_off_is_bit_equal():
    import torch

    A, B, seq, burn, n = 6, 3, 4, 2, 2
    batch, _ = _r2d2_batch(A, B, seq, burn, n, 8)
    assert float(batch.reward.abs().max()) > 100
    on = r2d2_agent(A, n, seq, burn, 1e-3)
    args = (batch.obs, batch.h0, batch.action, batch.reward, batch.terminal, batch.bootstrap, batch.seq_len)
    err = on.td_err(*args).detach().numpy()
    # the Q(s, a) columns as td_err unrolls them (r2d2.py td_err), then the target in float64
    with torch.no_grad():
        warm = {k: v[:burn] for k, v in batch.obs.items()}
        train = {k: v[burn:] for k, v in batch.obs.items()}
        _, on_hid = on.online_net.unroll_rnn(warm, batch.h0)
        _, tg_hid = on.target_net.unroll_rnn(warm, batch.h0)
        keep = (1 - batch.terminal.float()[burn - 1]).unsqueeze(0).unsqueeze(2)
        on_hid = {k: v * keep for k, v in on_hid.items()}
        tg_hid = {k: v * keep for k, v in tg_hid.items()}
        online_qa, greedy = on.online_net(train, on_hid, batch.action["a"][burn:])
        target_qa, _ = on.target_net(train, tg_hid, greedy)
    oq, tq = online_qa.double().numpy(), target_qa.double().numpy()
    r, b = batch.reward.double().numpy()[burn:], batch.bootstrap.double().numpy()[burn:]
    lens = batch.seq_len.numpy()
    ref = np.zeros((B, seq))
    plain = np.zeros((B, seq))
    for i in range(seq):
        pad = i >= lens - burn
        ref[:, i] = np.where(pad, 0.0, h64(r[i] + b[i] * (0.997 ** n * hinv64(tq[i + n], 1e-3)), 1e-3) - oq[i])
        plain[:, i] = np.where(pad, 0.0, r[i] + b[i] * (0.997 ** n * tq[i + n]) - oq[i])
    assert np.abs(ref - plain).max() > 10 and (ref == 0).any()
    np.testing.assert_allclose(err, ref, rtol=0, atol=AGENT_ATOL)
    per_seq, prio = on.loss(batch)
    ref_loss = np.where(np.abs(ref) < 1, 0.5 * ref * ref, np.abs(ref) - 0.5).sum(1)
    np.testing.assert_allclose(per_seq.detach().numpy(), ref_loss, rtol=0, atol=seq * AGENT_ATOL)
    masked = np.abs(ref) * (np.arange(seq)[None, :] < lens[:, None])
    ref_prio = 0.9 * masked.max(1) + (1 - 0.9) * masked.sum(1) / (lens - burn)
    np.testing.assert_allclose(prio.numpy(), ref_prio, rtol=1e-6, atol=AGENT_ATOL)
    # compute_priority: one K-row step from a recurrent state
    step = lambda t: {k: v[t] for k, v in batch.obs.items()}
    hid = {k: v.clone() for k, v in batch.h0.items()}
    pr = on.compute_priority(step(0), {"a": batch.action["a"][0]}, batch.reward[0], batch.terminal[0], batch.bootstrap[0],
                             step(n), hid, hid)
    with torch.no_grad():
        lift = lambda d: {k: v.unsqueeze(0) for k, v in d.items()}
        q0 = on.online_net(lift(step(0)), hid, batch.action["a"][0].unsqueeze(0))[0].squeeze(0).double().numpy()
        na = on.online_net.act(step(n), hid)[0].unsqueeze(0)
        bq = on.target_net(lift(step(n)), hid, na)[0].squeeze(0).double().numpy()
    ref_pr = np.abs(h64(batch.reward[0].double().numpy() + batch.bootstrap[0].double().numpy() * (0.997 ** n)
                        * hinv64(bq, 1e-3), 1e-3) - q0)
    np.testing.assert_allclose(pr.numpy(), ref_pr, rtol=0, atol=AGENT_ATOL)
    twin = type(on).clone(on, "cpu")
    assert twin.value_rescale == on.value_rescale and np.array_equal(twin.td_err(*args).detach().numpy(), err)
    zero, bare = r2d2_agent(A, n, seq, burn, 0.0), r2d2_agent(A, n, seq, burn, None)
    assert bare.value_rescale == 0.0
    for a, b_ in zip(zero.loss(batch), bare.loss(batch)):
        assert torch.equal(a, b_)
    assert torch.equal(zero.td_err(*args), bare.td_err(*args))
    np.testing.assert_allclose(bare.td_err(*args).detach().numpy(), plain, rtol=0, atol=AGENT_ATOL)
