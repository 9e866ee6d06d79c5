"""Functional CPU references of the two networks and the two losses, in any torch dtype (float64 is the ground truth the
precision modes are measured against).

rela_amd/pyrela casts observations with `.float()` (net.py: AtariFFNet.forward, AtariLSTMNet._features), so its modules
cannot simply be `.double()`-ed; these functions restate them with the cast as a parameter:
  ffnet_forward    AtariFFNet.forward                          (pyrela/net.py)
  lstmnet_step     one AtariLSTMNet step: trunk -> LSTM cell -> heads, as tests/test_lstmnet_gpu.py evaluates it
  apex_loss        ApexAgent.loss + (per_sample * w).mean().backward()  (pyrela/apex.py)
  r2d2_loss        R2D2Agent.loss + (per_seq * w).mean().backward()     (pyrela/r2d2.py)
They run on the CPU on purpose (no f64 convolutions on the GPU are involved) and are pinned to pyrela in float32 by
tests/test_f64_ref_cpu.py.  Parameters are dicts of state_dict keys -> numpy / torch tensors."""
import torch
import torch.nn.functional as F

FLAT, HIDDEN = 3136, 512


def params_as(p, dtype, requires_grad=False):
    out = {}
    for k, v in p.items():
        t = torch.as_tensor(v).detach().to("cpu", dtype).clone()
        out[k] = t.requires_grad_(requires_grad)
    return out


def _t(x, dtype):
    return torch.as_tensor(x).detach().to("cpu", dtype)


def trunk(p, s, dtype):
    """uint8 frames [N, 4, 84, 84] -> conv features [N, 3136] (net.py _conv_trunk on s / 255)"""
    x = torch.as_tensor(s).to("cpu").to(dtype) / 255.0
    x = F.relu(F.conv2d(x, p["net.0.weight"], p["net.0.bias"], stride=4))
    x = F.relu(F.conv2d(x, p["net.2.weight"], p["net.2.bias"], stride=2))
    x = F.relu(F.conv2d(x, p["net.4.weight"], p["net.4.bias"], stride=1))
    return x.flatten(1)


def dueling(v, a, legal, dim):
    masked = a * legal
    return v + masked - masked.mean(dim, keepdim=True)


def ffnet_forward(p, s, legal, dtype):
    """Q [N, A] of AtariFFNet; p already in `dtype` (params_as)"""
    hid = F.relu(F.linear(trunk(p, s, dtype), p["linear.0.weight"], p["linear.0.bias"]))
    return dueling(F.linear(hid, p["fc_v.weight"], p["fc_v.bias"]), F.linear(hid, p["fc_a.weight"], p["fc_a.bias"]),
                   _t(legal, dtype), 1)


def lstm_cell(p, x, h, c):
    """torch.nn.LSTM's cell, gate order i, f, g, o"""
    g = F.linear(x, p["lstm.weight_ih_l0"], p["lstm.bias_ih_l0"]) + F.linear(h, p["lstm.weight_hh_l0"], p["lstm.bias_hh_l0"])
    i, f, gg, o = g.chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def lstmnet_step(p, s, legal, h, c, dtype):
    """-> h, c, q, adv [N, ...] of one AtariLSTMNet step from the state (h, c)"""
    with torch.no_grad():
        pp = params_as(p, dtype)
        h, c = lstm_cell(pp, trunk(pp, s, dtype), _t(h, dtype), _t(c, dtype))
        adv = F.linear(h, pp["fc_a.weight"], pp["fc_a.bias"])
        q = dueling(F.linear(h, pp["fc_v.weight"], pp["fc_v.bias"]), adv, _t(legal, dtype), 1)
    return h, c, q, adv


def _greedy(q, legal, dim):
    """masked arg-max; the shift uses the minimum of the WHOLE tensor (apex.py masked_greedy, net.py forward)"""
    return ((1 + q - q.min()) * legal).argmax(dim)


def apex_loss(p_on, p_tg, batch, weight, gamma, multi_step, dtype):
    """-> (loss, priority [B], per_sample [B], {key: grad of the online parameters}) of ApexAgent.loss with the loss
    (per_sample * weight).mean(); batch as tests/test_learner_gpu.py:make_batch builds it (any device)"""
    on, tg = params_as(p_on, dtype, True), params_as(p_tg, dtype)
    obs, nobs = batch.obs, batch.next_obs
    a = batch.action["a"].cpu()
    q_taken = ffnet_forward(on, obs["s"].cpu(), obs["legal_move"].cpu(), dtype).gather(1, a.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        nlegal = _t(nobs["legal_move"].cpu(), dtype)
        next_a = _greedy(ffnet_forward(on, nobs["s"].cpu(), nlegal, dtype), nlegal, 1)
        next_q = ffnet_forward(tg, nobs["s"].cpu(), nlegal, dtype).gather(1, next_a.unsqueeze(1)).squeeze(1)
        target = _t(batch.reward.cpu(), dtype) + _t(batch.bootstrap.cpu(), dtype) * (gamma ** multi_step) * next_q
    err = target - q_taken
    per_sample = F.smooth_l1_loss(err, torch.zeros_like(err), reduction="none")
    loss = (per_sample * _t(weight.cpu(), dtype)).mean()
    loss.backward()
    return loss.detach(), err.detach().abs(), per_sample.detach(), {k: v.grad for k, v in on.items()}


def _unroll(p, s, legal, h, c, dtype, hooks=None, t0=0):
    """[T, B, ...] frames from the state (h, c) [B, 512] -> (q [T, B, A], h, c): AtariLSTMNet.unroll_rnn + dueling heads.
    hooks (optional, for tests that restate a defect; t0 = the batch's time index of s[0]):
      "trunk": f(p, frames, dtype) in place of trunk;  "state": f(t0 + t, h, c) -> (h, c) entering step t0 + t"""
    hooks = hooks or {}
    T, B = s.shape[:2]
    x = hooks.get("trunk", trunk)(p, s.reshape(T * B, *s.shape[2:]), dtype).view(T, B, FLAT)
    outs = []
    for t in range(T):
        if "state" in hooks:
            h, c = hooks["state"](t0 + t, h, c)
        h, c = lstm_cell(p, x[t], h, c)
        outs.append(h)
    o = torch.stack(outs) if T else x.new_zeros(0, B, HIDDEN)
    q = dueling(F.linear(o, p["fc_v.weight"], p["fc_v.bias"]), F.linear(o, p["fc_a.weight"], p["fc_a.bias"]), legal, 2)
    return q, h, c


def r2d2_loss(p_on, p_tg, batch, weight, gamma, multi_step, eta, seq_len, burn_in, dtype, hooks=None):
    """-> (loss, priority [B], loss per sequence [B], {key: grad of the online parameters}) of R2D2Agent.loss with the
    loss (per_seq * weight).mean(); batch RNNTransition-shaped, time-major (tests/test_r2d2_learner_gpu.py).
    hooks (optional, for tests that restate a defect; net = "online" | "target", t = time index in the batch):
      "trunk": f(net, p, frames, dtype) in place of trunk (a parameter it never uses gets the gradient None)
      "state": f(net, t, h, c) -> (h, c) entering step t
      "keep": f(keep [B, 1]) -> the factor on the state after the burn-in
      "per_seq": f(per_seq [B]) -> the losses that enter the weighted mean (the returned ones stay as computed)"""
    hooks = hooks or {}

    def hk(net):
        out = {}
        if "trunk" in hooks:
            out["trunk"] = lambda p, frames, dt: hooks["trunk"](net, p, frames, dt)
        if "state" in hooks:
            out["state"] = lambda t, h, c: hooks["state"](net, t, h, c)
        return out

    on, tg = params_as(p_on, dtype, True), params_as(p_tg, dtype)
    s = batch.obs["s"].cpu()
    legal = _t(batch.obs["legal_move"].cpu(), dtype)
    h0, c0 = _t(batch.h0["h0"].cpu(), dtype)[0], _t(batch.h0["c0"].cpu(), dtype)[0]
    terminal = _t(batch.terminal.cpu(), dtype)
    lens = _t(batch.seq_len.cpu(), dtype)
    b = burn_in
    if b == 0:
        hon, con, htg, ctg = h0, c0, h0, c0
    else:
        with torch.no_grad():
            _, hon, con = _unroll(on, s[:b], legal[:b], h0, c0, dtype, hk("online"))
            _, htg, ctg = _unroll(tg, s[:b], legal[:b], h0, c0, dtype, hk("target"))
        keep = (1 - terminal[b - 1]).unsqueeze(1)  # dummy burn-in at an episode's start
        if "keep" in hooks:
            keep = hooks["keep"](keep)
        hon, con, htg, ctg = hon * keep, con * keep, htg * keep, ctg * keep
    q_on, _, _ = _unroll(on, s[b:], legal[b:], hon, con, dtype, hk("online"), b)
    a_train = batch.action["a"].cpu()[b:]
    online_qa = q_on.gather(2, a_train.unsqueeze(2)).squeeze(2)
    with torch.no_grad():
        greedy = _greedy(q_on, legal[b:], 2)
        q_tg, _, _ = _unroll(tg, s[b:], legal[b:], htg, ctg, dtype, hk("target"), b)
        target_qa = q_tg.gather(2, greedy.unsqueeze(2)).squeeze(2)
    reward, boot = _t(batch.reward.cpu(), dtype)[b:], _t(batch.bootstrap.cpu(), dtype)[b:]
    gamma_n = gamma ** multi_step
    cols = []
    for i in range(seq_len):
        target = reward[i] + boot[i] * (gamma_n * target_qa[i + multi_step])
        pad = (i >= (lens - b)).to(dtype)
        cols.append((target - online_qa[i]) * (1 - pad))
    err = torch.stack(cols, 1)
    per_seq = F.smooth_l1_loss(err, torch.zeros_like(err), reduction="none").sum(1)
    loss = (hooks["per_seq"](per_seq) if "per_seq" in hooks else per_seq) * _t(weight.cpu(), dtype)
    loss = loss.mean()
    loss.backward()
    with torch.no_grad():
        pr = err.abs()
        t = torch.arange(pr.size(1))
        masked = pr * (t.unsqueeze(0) < lens.unsqueeze(1)).to(dtype)
        prio = eta * masked.max(1)[0] + (1.0 - eta) * masked.sum(1) / (lens - b)
    return loss.detach(), prio, per_seq.detach(), {k: v.grad for k, v in on.items()}


def err_stats(got, ref):
    """(max, mean) |got - ref| in float64"""
    d = (torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(ref).detach().cpu().double()).abs()
    return float(d.max()), float(d.mean())


def rel_fro(got, ref):
    """||got - ref||_F / ||ref||_F in float64"""
    g, r = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((g - r).norm()) / (float(r.norm()) + 1e-300)
