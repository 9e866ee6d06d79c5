"""tests/f64_ref.py against rela_amd/pyrela in float32 on the CPU: the functional restatements the GPU accuracy tests
measure every precision mode against must compute what the reference's modules compute.  In float32 they run the same
torch operations, so the tolerance is tight; in float64 they must agree with the float32 modules to f32 rounding."""
import numpy as np
import pytest

import f64_ref as R

TIGHT = dict(rtol=1e-5, atol=1e-6)


def _close(got, ref, tight=True, what=""):
    got, ref = got.detach().double().numpy(), ref.detach().double().numpy()
    scale = float(np.abs(ref).max()) + 1e-30
    if tight:
        np.testing.assert_allclose(got, ref, rtol=TIGHT["rtol"], atol=TIGHT["atol"] * max(1.0, scale), err_msg=what)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * scale, err_msg=what)


@pytest.mark.parametrize("scale", [1.0, 4.6])
def test_ffnet_forward_matches_pyrela(scale):
    import torch

    from rela_amd.pyrela.net import AtariFFNet
    from synth import synth_obs, synth_params

    A, N = 18, 6
    p = synth_params(A, 3, scale)
    net = AtariFFNet(A)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    s = synth_obs(N, 4)
    legal = (np.random.default_rng(1).uniform(size=(N, A)) < 0.7).astype(np.float32)
    with torch.no_grad():
        ref = net({"s": torch.from_numpy(s), "legal_move": torch.from_numpy(legal)})
        for dtype, tight in ((torch.float32, True), (torch.float64, False)):
            q = R.ffnet_forward(R.params_as(p, dtype), s, legal, dtype)
            assert q.dtype == dtype
            _close(q, ref, tight, str(dtype))


@pytest.mark.parametrize("scale", [1.0, 4.6])
def test_lstmnet_step_matches_pyrela(scale):
    """(x 4.6: gate pre-activations of ~50, whose f32 rounding in torch.nn.LSTM's fused sums moves h by ~2e-5: the f32
    comparison there is at the GPU parity tests' 1e-4)"""
    import torch

    from rela_amd.pyrela.net import AtariLSTMNet, dueling_q
    from synth import synth_lstm_params, synth_obs

    A, N = 6, 5
    p = {k: (v * scale).astype(np.float32) for k, v in synth_lstm_params(A, 8).items()}
    rng = np.random.default_rng(2)
    s = synth_obs(N, 9)
    legal = (rng.uniform(size=(N, A)) < 0.8).astype(np.float32)
    h_in = rng.normal(0, 0.3, (N, 512)).astype(np.float32)
    c_in = rng.normal(0, 0.5, (N, 512)).astype(np.float32)
    net = AtariLSTMNet("cpu", A)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    with torch.no_grad():
        x = net._features(torch.from_numpy(s)).unsqueeze(0)
        o, (hr, cr) = net.lstm(x, (torch.from_numpy(h_in).unsqueeze(0), torch.from_numpy(c_in).unsqueeze(0)))
        adv_r = net.fc_a(o).squeeze(0)
        q_r = dueling_q(net.fc_v(o), net.fc_a(o), torch.from_numpy(legal).unsqueeze(0), 2).squeeze(0)
    for dtype, tight in ((torch.float32, scale == 1.0), (torch.float64, False)):
        h, c, q, adv = R.lstmnet_step(p, s, legal, h_in, c_in, dtype)
        for got, ref, name in ((h, hr.squeeze(0), "h"), (c, cr.squeeze(0), "c"), (q, q_r, "q"), (adv, adv_r, "adv")):
            _close(got, ref, tight, "%s %s" % (name, dtype))


def test_apex_loss_matches_pyrela():
    import torch

    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet
    from test_learner_gpu import make_batch

    A, B, n, gamma = 6, 12, 3, 0.99
    torch.manual_seed(4)
    agent = ApexAgent(lambda: AtariFFNet(A), n, gamma)
    with torch.no_grad():
        for p in agent.target_net.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    batch, w = make_batch(B, A, 5, device="cpu")
    per_sample, prio = agent.loss(batch, sync_priority=False)
    loss = (per_sample * w).mean()
    loss.backward()
    p_on = {k: v.detach() for k, v in agent.online_net.state_dict().items()}
    p_tg = {k: v.detach() for k, v in agent.target_net.state_dict().items()}
    for dtype, tight in ((torch.float32, True), (torch.float64, False)):
        l_, pr_, ps_, grads = R.apex_loss(p_on, p_tg, batch, w, gamma, n, dtype)
        _close(l_, loss, tight, "loss")
        _close(pr_, prio, tight, "priority")
        _close(ps_, per_sample, tight, "per_sample")
        assert set(grads) == set(p_on)
        for key, prm in agent.online_net.named_parameters():
            _close(grads[key], prm.grad, tight, "grad %s %s" % (key, dtype))


@pytest.mark.parametrize("A,B,seq,burn,n", [(6, 4, 5, 3, 2), (6, 3, 4, 0, 2)])
def test_r2d2_loss_matches_pyrela(A, B, seq, burn, n):
    """(with and without burn-in; _random_batch starts some sequences at an episode's start: dummy burn-in, padding)"""
    import torch

    from test_r2d2_learner_gpu import _agent, _random_batch

    gamma, eta = 0.997, 0.9
    agent = _agent(A, n, gamma, eta, seq, burn, 71, 72, "cpu")
    batch, w = _random_batch(np.random.default_rng(7), A, B, seq, burn, n, "cpu")
    per_seq, prio = agent.loss(batch, sync_priority=False)
    loss = (per_seq * w).mean()
    loss.backward()
    p_on = {k: v.detach() for k, v in agent.online_net.state_dict().items()}
    p_tg = {k: v.detach() for k, v in agent.target_net.state_dict().items()}
    for dtype, tight in ((torch.float32, True), (torch.float64, False)):
        l_, pr_, ls_, grads = R.r2d2_loss(p_on, p_tg, batch, w, gamma, n, eta, seq, burn, dtype)
        _close(l_, loss, tight, "loss")
        _close(pr_, prio, tight, "priority")
        _close(ls_, per_seq, tight, "loss_seq")
        assert set(grads) == set(p_on)
        for key, prm in agent.online_net.named_parameters():
            _close(grads[key], prm.grad, tight, "grad %s %s" % (key, dtype))
