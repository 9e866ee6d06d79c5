"""Float64 references of the two stages of the R2D2 learner's backward pass that sit between the Q tables and the BPTT, one
call at a time (include/rela_amd.h, csrc/learner_r2d2.hip):

  rela_debug_seq_loss_grad       seq_reference: the learner's restatement of R2D2Agent.td_err / loss / aggregate_priority
                                 (pyrela/r2d2.py:103-206) and of AtariLSTMNet.forward's greedy rule and duel (pyrela/net.py:
                                 93-99, 157-162), from the Q tables of the time-major training rows (row = i * batch + b)
  rela_debug_seq_head_backward   head_reference:  d_o = d_ha[:, :A] @ fc_a_w + d_ha[:, 31:] @ fc_v_w,  the two weight
                                 gradients d_ha.T @ o, the two bias gradients as column sums (no ReLU: o is the LSTM's output)

Plain numpy / torch float64, none of the project's kernels; tests/test_seq_loss_ref_cpu.py pins both to float64 autograd,
proves the properties of the inputs at every shape of the GPU test and shows which restated defects the checks catch.

THE GREEDY RULE IS DECIDED IN FLOAT32: fl(fl(1 + q) - min) * legal can tie where the float64 values differ, so greedy_f32
evaluates it in numpy float32 in the kernel's operation order, and check_loss_inputs asserts that the float64 argmax agrees
on every row (the tables are dyadic, so here the float32 evaluation is exact; `tie` rows tie in both).

All bounds are DERIVED below from the count of roundings (u = 2^-24, float32's unit roundoff, -ffp-contract=off: no fused
multiply-add), never taken from a kernel's output."""
import functools

import numpy as np
import torch

from trunk_bwd_ref import U_F32, err_units, rel_fro  # noqa: F401

GAMMA_N = 0.5
ETA = 0.9
GRID = 2.0 ** -5
Q_MIN = -64.0            # the global minimum of q_on: far below every other entry (those lie above -34)
Q_DEEP = -32.0           # offset of a `deep` row: 1 + q - min stays positive only with the TRUE minimum
Q_TG_LOW = -2.0 ** 21    # below Q_MIN, in q_tg only: a minimum taken over q_tg too collapses 1 + q - min to multiples of 1/4
Q_TG_HUGE = 1e30         # the target Q of a `boot0_huge` step: finite, and multiplied by bootstrap = 0
BIG_WEIGHT = 8.0

SEQ_ROLES = ("full", "burn_plus_1", "full_minus_1", "middle", "weight_0", "big_weight")  # by b mod 6
# live rows in table order, by their running index mod 10
ROW_ROLES = ("dyadic_plus1", "dyadic_minus1", "dyadic_0", "large_pos", "large_neg", "tie", "illegal_best", "single_legal",
             "boot0_huge", "act_last")
MIN_PLACES = ("last", "i1023", "i1024")  # `last` is also `in a padded row`: the last row of the table is always padded

# (batch, seq_len, burn_in, multi_step) of tests/test_seq_loss_gpu.py; A over A_LIST at RAGGED, 18 elsewhere
RAGGED = (33, 12, 6, 3)
LOSS_SHAPES = ((1, 1, 0, 1), (5, 7, 0, 2), RAGGED, (64, 5, 2, 2), (65, 5, 2, 2), (1023, 3, 1, 1), (1024, 3, 1, 1))
A_LIST = (1, 6, 18, 31)
LOSS_CASES = [(s, A) for s in LOSS_SHAPES for A in (A_LIST if s == RAGGED else (18,))]
VR_EPS = (0.0, 1e-3)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def seq_lengths(batch, seq, burn):
    """sequence lengths by role (burn-in included); every length keeps seq_len_b - burn_in >= 1: the replay never emits
    less, and with 0 both sides divide by zero"""
    by_role = {"full": burn + seq, "burn_plus_1": burn + 1, "full_minus_1": burn + max(1, seq - 1),
               "middle": burn + max(1, (seq + 1) // 2), "weight_0": burn + seq, "big_weight": burn + max(1, seq // 3)}
    return np.array([by_role[SEQ_ROLES[b % 6]] for b in range(batch)], np.float32)


def row_roles(batch, seq, burn, n):
    """-> list over the (seq + n) * batch rows: a ROW_ROLES name for a live row (i < seq_len_b - burn_in, which implies
    i < seq), "padded" for every other row"""
    live_len = seq_lengths(batch, seq, burn) - burn
    out, k = [], 0
    for i in range(seq + n):
        for b in range(batch):
            if i < live_len[b]:
                out.append(ROW_ROLES[k % len(ROW_ROLES)])
                k += 1
            else:
                out.append("padded")
    return out


DEEP_SAFE = ("dyadic_plus1", "dyadic_minus1", "dyadic_0", "large_pos", "large_neg", "act_last", "boot0_huge")


def deep_row(roles, A):
    """the last live row whose role leaves its legal moves free (DEEP_SAFE) becomes a `deep` row on top of its role, when it
    starts beyond flat index 1024 and A >= 2: all its online Q lie near Q_DEEP, column 0 is illegal.  With the true minimum
    (1 + q - min) * legal is positive on its legal actions; with a minimum that skips the tail of the table it is negative
    there and column 0 wins."""
    live = [r for r, role in enumerate(roles) if role in DEEP_SAFE and r * A >= 1025]
    return live[-1] if A >= 2 and live else None


# ---- the reference -------------------------------------------------------------------------------------------------------------
def greedy_f32(q_on, q_tg, legal, defect=None):
    """seq_select's rule in numpy float32, in the kernel's operation order: first maximum of ((1 + q) - min) * legal"""
    f = np.float32
    q_on, legal = np.asarray(q_on, f), np.asarray(legal, f)
    A = q_on.shape[1]
    mn = q_on.min()
    if defect == "min_first_1024":
        mn = q_on.reshape(-1)[:1024].min()
    if defect == "min_with_q_tg":
        mn = min(mn, np.asarray(q_tg, f).min())
    v = ((f(1.0) + q_on) - mn) * (np.ones_like(legal) if defect == "argmax_ignores_legal" else legal)
    if defect == "last_max":
        return (A - 1) - v[:, ::-1].argmax(1)
    return v.argmax(1)


def greedy_f64(q_on, legal):
    q = np.asarray(q_on, np.float64)
    return ((1.0 + q - q.min()) * np.asarray(legal, np.float64)).argmax(1)


def loss_args(inp):
    return {k: inp[k] for k in ("A", "batch", "seq", "burn", "n", "q_on", "q_tg", "legal", "act", "reward", "bootstrap",
                                "seq_lens", "weight")}


def seq_reference(A, batch, seq, burn, n, q_on, q_tg, legal, act, reward, bootstrap, seq_lens, weight, gamma_n=GAMMA_N,
                  eta=ETA, e=None, defect=None):
    """float64 from the float32 tables (value rescaling off); rows are time-major.  e [seq][batch]: the TD errors to
    continue from (the kernel's own float32 ones, for the bounds that count the roundings AFTER e); defect: one of DEFECTS.
    -> dict of numpy float64 arrays: greedy, qa_on, qa_tg, dqa [rows]; e, target, mag [seq][batch]; loss_seq, priority,
    terms (loss_seq * w) [batch]; loss; d_ha [rows][32]"""
    f8 = lambda x: np.asarray(x, np.float64)
    rows = (seq + n) * batch
    q_on, q_tg, legal = (f8(t).reshape(rows, A) for t in (q_on, q_tg, legal))
    act = np.asarray(act).astype(np.int64).reshape(rows)
    reward, bootstrap = f8(reward).reshape(seq + n, batch), f8(bootstrap).reshape(seq + n, batch)
    lens, w = f8(seq_lens), f8(weight)
    r = np.arange(rows)
    greedy = greedy_f32(q_on, q_tg, legal, defect)                                   # net.py:160-162
    qa_on = q_on[r, act]                                                             # net.py:157
    qa_tg = q_tg[r, greedy]
    off = n - 1 if defect == "target_row_n_minus_1" else n
    qt = qa_tg.reshape(seq + n, batch)[off:off + seq]                                # r2d2.py:173-174: row i + multi_step
    boot_q = bootstrap[:seq] * (gamma_n * qt)
    target = reward[:seq] + boot_q                                                   # :175-176
    i = np.arange(seq, dtype=np.float64)[:, None]
    pad = i >= (lens - burn)[None, :]                                                # should_padding :179
    if defect == "pad_mask_gt":
        pad = i > (lens - burn)[None, :]
    if defect == "pad_mask_seq_len":
        pad = i >= lens[None, :]
    qo = qa_on.reshape(seq + n, batch)[:seq]
    mag = np.abs(reward[:seq]) + np.abs(boot_q) + np.abs(qo)
    if e is None:
        e = np.where(pad, 0.0, target - qo)                                          # :184
    else:
        e = f8(e).reshape(seq, batch)
    ae = np.abs(e)
    loss_seq = np.where(ae < 1, 0.5 * e * e, ae - 0.5).sum(0)                        # smooth_l1, summed over the sequence :199-204
    pmask = np.ones_like(ae) if defect == "priority_mask_dropped" else (i < lens[None, :]).astype(np.float64)  # :113-115
    masked = ae * pmask
    mean = masked.sum(0) / (lens if defect == "mean_over_seq_len" else lens - burn)  # :117
    # (1.0 - eta) is folded in double and the result becomes a float32 constant of the kernel, as the actor's r2d2_aggregate
    one_minus = float(np.float32(1.0 - eta))
    if defect == "one_minus_eta_f32":
        one_minus = float(np.float32(1.0) - np.float32(eta))
    priority = float(np.float32(eta)) * masked.max(0) + one_minus * mean             # :118-119
    terms = loss_seq * w
    loss = terms.sum() / (1024.0 if defect == "loss_mean_over_1024" else batch)      # main.py: (loss * weight).mean()
    g = np.where(pad, 0.0, -w[None, :] * np.clip(e, -1, 1) / batch)
    dqa = np.concatenate([g.reshape(-1), np.zeros(n * batch)])
    ind = np.zeros((rows, A))
    ind[r, act] = 1
    div = np.maximum(legal.sum(1, keepdims=True), 1) if defect == "one_over_num_legal" else float(A)
    d_ha = np.zeros((rows, 32))
    d_ha[:, :A] = legal * (dqa[:, None] * (ind - 1.0 / div))                         # duel, net.py:93-99
    d_ha[:, A if defect == "value_in_column_A" else 31] = dqa
    return {"greedy": greedy, "qa_on": qa_on, "qa_tg": qa_tg, "target": target, "mag": mag, "e": e, "pad": pad,
            "loss_seq": loss_seq, "priority": priority, "terms": terms, "loss": loss, "dqa": dqa, "d_ha": d_ha}


def e_f32(inp, greedy, vr_eps):
    """seq_td_loss's e in numpy float32, every operation in the kernel's order; the rescaling through the host build of
    csrc/value_rescale.h (tests/value_rescale_util.py).  -> float32 [seq][batch]"""
    from value_rescale_util import host_h_hinv

    f = np.float32
    A, B, seq, burn, n = (inp[k] for k in ("A", "batch", "seq", "burn", "n"))
    rows = (seq + n) * B
    r = np.arange(rows)
    qa_on = inp["q_on"].reshape(rows, A)[r, inp["act"]].reshape(seq + n, B)[:seq]
    qt = inp["q_tg"].reshape(rows, A)[r, greedy].reshape(seq + n, B)[n:n + seq]
    reward, boot = inp["reward"].reshape(seq + n, B)[:seq], inp["bootstrap"].reshape(seq + n, B)[:seq]
    if vr_eps > 0:
        hinv = host_h_hinv(qt, vr_eps)[1].reshape(qt.shape)
        target = host_h_hinv(reward + boot * (f(GAMMA_N) * hinv), vr_eps)[0].reshape(qt.shape)
    else:
        target = reward + boot * (f(GAMMA_N) * qt)
    pad = np.arange(seq, dtype=f)[:, None] >= (inp["seq_lens"] - f(burn))[None, :]
    return np.where(pad, f(0), target - qa_on).astype(f)


def td_loss_f32(inp, e32, eta=ETA):
    """seq_td_loss and seq_head_grad after e, in numpy float32 with every operation in the kernels' order (sequential sums
    over the steps, the 1024-lane tree of the loss, correctly rounded divisions): -> float32 dqa [rows], loss_seq, priority
    [batch], loss [1], d_ha [rows][32].  The bits the kernels must produce if their e is e32."""
    f = np.float32
    A, B, seq, burn, n = (inp[k] for k in ("A", "batch", "seq", "burn", "n"))
    rows = (seq + n) * B
    lens, w = inp["seq_lens"].astype(f), inp["weight"].astype(f)
    inv_b = f(1.0) / f(B)
    lsum, psum, pmax = np.zeros(B, f), np.zeros(B, f), np.zeros(B, f)
    dqa = np.zeros((seq + n, B), f)
    for i in range(seq):
        e = e32[i].astype(f)
        ae = np.abs(e)
        pad = f(i) >= lens - f(burn)
        lsum = lsum + np.where(ae < f(1.0), (f(0.5) * e) * e, ae - f(0.5))
        pm = np.where(f(i) < lens, ae, f(0))
        psum = psum + pm
        pmax = np.maximum(pmax, pm)
        dqa[i] = np.where(pad, f(0), (-(w * np.clip(e, f(-1.0), f(1.0)))) * inv_b)
    priority = f(eta) * pmax + f(1.0 - eta) * (psum / (lens - f(burn)))
    red = np.zeros(1024, f)
    red[:B] = lsum * w
    o = 512
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    loss = np.array([red[0] / f(B)], f)
    dqa = dqa.reshape(rows)
    ind = np.zeros((rows, A), f)
    ind[np.arange(rows), inp["act"]] = 1
    d_ha = np.zeros((rows, 32), f)
    d_ha[:, :A] = inp["legal"].reshape(rows, A) * (dqa[:, None] * (ind - f(1.0) / f(A)))
    d_ha[:, 31] = dqa
    return {"dqa": dqa, "loss_seq": lsum, "priority": priority.astype(f), "loss": loss, "d_ha": d_ha}


# ---- DERIVED bounds of the loss tap, u = 2^-24 per rounding, (1 + u)^k - 1 for k roundings in a row ----------------------------
def _k(k):
    return (1.0 + U_F32) ** k - 1.0


# e = fl(fl(r + fl(boot * fl(gamma_n * qt))) - qa): the two products, the sum and the difference -- four roundings of
# quantities no larger than mag = |r| + |boot * gamma_n * qt| + |qa|
E_ROUNDINGS = 4


def e_bound(ref):
    return _k(E_ROUNDINGS) * ref["mag"]


# from the kernel's own e:  g = -(w * clamp(e)) * fl(1 / B): the product, fl(1 / B), the second product -- three roundings;
# column 31 of d_ha is g.  Column k < A = legal * (g * (ind - fl(1 / A))): fl(1 / A), the subtraction, the product -- three
# more (legal is 0 or 1: exact), |ind - 1 / A| <= 1.
DQA_ROUNDINGS, D_HA_ROUNDINGS = 3, 6


def dqa_bound(after):
    return _k(DQA_ROUNDINGS) * np.abs(after["dqa"])


def d_ha_bound(after):
    return _k(D_HA_ROUNDINGS) * np.abs(after["dqa"])[:, None]


# loss_seq from the kernel's own e: a term is fl(fl(0.5 * e) * e) (the halving is exact) or fl(|e| - 0.5): ONE rounding;
# the sequence's seq terms are added one after the other to 0: seq additions.  All terms >= 0, so every partial sum is
# within its roundings of the exact one: seq + 1 roundings of sum(terms).
def loss_seq_roundings(seq):
    return seq + 1


# priority from the kernel's own e: |e| is exact; the masked sum is seq additions; len - burn is exact (small integers);
# the division, one_minus_eta * mean, eta * max and the final sum: four more.  eta and one_minus_eta are the kernel's float32
# constants in the reference too.  All terms >= 0: seq + 4 roundings of the priority.
def priority_roundings(seq):
    return seq + 4


# loss from the kernel's own e: a lane's term is fl(loss_seq * w) -- loss_seq's seq + 1 roundings and the product; the
# 1024-lane tree adds ten levels (adding the zeros of the idle lanes is exact); B as a float is exact, the division rounds
# once.  All terms >= 0: (seq + 1) + 1 + 10 + 1 roundings of sum(terms) / B.
def loss_roundings(seq):
    return (seq + 1) + 1 + 10 + 1


# a sequence of length burn_in + 1 has one live step: max = mean = |e_0| and priority = fl(fl(eta * a) + fl(one_minus_eta *
# fl(a / 1))).  The check is |priority - |e_0|| <= 2 u |e_0|.  (By count: the two constants sum to 1 - 0.375 u, the two
# products round once each on 0.9 a and 0.1 a, the sum once on a: 2.4 u |e_0| in the worst case; 2 u is what is asserted.)
ONE_STEP_PRIORITY_UNITS = 2.0


# ---- the inputs of the loss tap --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def loss_inputs(batch, A, seq, burn, n, min_at="last", seed=5):
    """float32 tables and batch fields by role; check_loss_inputs asserts what the GPU test relies on.  Every table entry is
    on the 2^-5 grid (the float32 greedy rule is then exact), a row of a table is a permutation of a stretch of the grid (its
    entries differ by at least 2^-5); rewards put e into the class of the row's role; gamma_n = 0.5."""
    rng = np.random.default_rng(seed + 1000 * batch + 10 * A + seq)
    f = np.float32
    rows = (seq + n) * batch
    roles = row_roles(batch, seq, burn, n)
    lens = seq_lengths(batch, seq, burn)

    def table():
        t = np.stack([rng.permutation(A) for _ in range(rows)]) + rng.integers(-64, 64, (rows, 1))
        return t.astype(np.float64) * GRID

    q_on, q_tg = table(), table()
    legal = (rng.uniform(size=(rows, A)) < 0.7).astype(f)
    act = rng.integers(0, A, rows).astype(np.int64)
    legal[np.arange(rows), act] = 1
    boot = (rng.uniform(size=rows) < 0.8).astype(f)
    deep = deep_row(roles, A)
    for r, role in enumerate(roles):
        if role == "padded":  # as padLike leaves a slot: no legal action, action 0; the nets still produce Q-values
            legal[r], act[r], boot[r] = 0, 0, 0
            continue
        if role.startswith("dyadic"):
            boot[r] = 1
        if role == "act_last":
            act[r] = A - 1
            legal[r, A - 1] = 1
        if role == "single_legal":
            legal[r] = 0
            legal[r, act[r]] = 1
        if role == "tie" and A >= 2:  # two legal actions with equal online Q above the rest: the first must win
            j1, j2 = sorted(rng.choice(A, 2, replace=False))
            legal[r, j1] = legal[r, j2] = 1
            q_on[r, j1] = q_on[r, j2] = q_on[r].max() + 4 * GRID
        if role == "illegal_best" and A >= 2:  # the largest online Q on an illegal action
            j = (act[r] + 1 + rng.integers(0, A - 1)) % A
            legal[r, j] = 0
            q_on[r, j] = q_on[r].max() + 4 * GRID
        if role == "boot0_huge":  # bootstrap 0 and a huge finite target Q in the row this step bootstraps from
            boot[r] = 0
            q_tg[r + n * batch] = Q_TG_HUGE * (1 + np.arange(A) / 1024.0)
        if r == deep:
            q_on[r] += Q_DEEP
            if act[r] == 0:
                act[r] = A - 1
            legal[r, 0], legal[r, act[r]] = 0, 1
    place = {"last": rows * A - 1, "i1023": 1023, "i1024": 1024}[min_at]
    assert place < rows * A, "the table has no element %d" % place
    q_on.reshape(-1)[place] = Q_MIN
    if A >= 2:  # never gathered: the last row is padded, its greedy action and its action are 0
        q_tg[rows - 1, A - 1] = Q_TG_LOW
    q_on, q_tg = q_on.astype(f), q_tg.astype(f)
    weight = rng.uniform(0.2, 1.0, batch).astype(f)
    for b in range(batch):
        weight[b] = {"weight_0": 0.0, "big_weight": BIG_WEIGHT}.get(SEQ_ROLES[b % 6], weight[b])
    inp = {"A": A, "batch": batch, "seq": seq, "burn": burn, "n": n, "q_on": q_on, "q_tg": q_tg, "legal": legal, "act": act,
           "reward": np.zeros(rows, f), "bootstrap": boot, "seq_lens": lens, "weight": weight}
    minus = -seq_reference(**loss_args(inp))["e"].reshape(-1)  # e = reward - minus on the live rows
    reward = rng.uniform(-1, 1, rows)
    for r, role in enumerate(roles[:seq * batch]):
        if role == "padded":
            continue
        if role.startswith("dyadic"):
            want = {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[role]
        elif role.startswith("large"):
            want = (1.0 if role == "large_pos" else -1.0) * rng.uniform(1.15, 3.0)
        else:
            want = rng.uniform(-0.85, 0.85)
        reward[r] = want + minus[r]
    inp["reward"] = reward.astype(f)
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


def roles_present(inp):
    """the roles the inputs hold (check_loss_inputs asserts the properties of each); tests/test_seq_loss_ref_cpu.py lists
    which shapes are too small for which"""
    A, batch, seq, burn, n = (inp[k] for k in ("A", "batch", "seq", "burn", "n"))
    roles = row_roles(batch, seq, burn, n)
    out = set(roles) | {SEQ_ROLES[b % 6] for b in range(batch)}
    if A < 2:
        out -= {"tie", "illegal_best"}
    else:
        out.add("q_tg_below_min")
    if deep_row(roles, A) is not None:
        out.add("deep")
    return out


def check_loss_inputs(inp, min_at="last"):
    """the properties the GPU test relies on, asserted on the data and its float64 reference; -> the reference"""
    A, batch, seq, burn, n = (inp[k] for k in ("A", "batch", "seq", "burn", "n"))
    rows = (seq + n) * batch
    roles = row_roles(batch, seq, burn, n)
    ref = seq_reference(**loss_args(inp))
    q_on, q_tg, legal, act = inp["q_on"], inp["q_tg"], inp["legal"], inp["act"]
    lens = inp["seq_lens"]
    assert bool((lens - burn >= 1).all()) and bool((lens <= burn + seq).all())
    for b in range(batch):
        role = SEQ_ROLES[b % 6]
        assert lens[b] == {"full": burn + seq, "burn_plus_1": burn + 1, "weight_0": burn + seq}.get(role, lens[b]), b
        assert inp["weight"][b] == {"weight_0": 0.0, "big_weight": BIG_WEIGHT}.get(role, inp["weight"][b]), b
    # the tables are dyadic: the float32 greedy rule is exact and agrees with float64 on EVERY row (tie rows tie in both)
    for t in (q_on, q_tg):
        fin = np.abs(t) < 1e20
        assert bool((t[fin] / GRID == np.round(t[fin] / GRID)).all())
    assert np.array_equal(ref["greedy"], greedy_f64(q_on, legal))
    # the global minimum sits where the case says, alone, and q_tg holds something smaller
    flat = q_on.reshape(-1)
    place = {"last": rows * A - 1, "i1023": 1023, "i1024": 1024}[min_at]
    assert flat[place] == Q_MIN and int(flat.argmin()) == place and int((flat == Q_MIN).sum()) == 1
    assert float(np.delete(flat, place).min()) >= Q_DEEP - 3.0
    assert roles[-1] == "padded" and (min_at != "last" or roles[place // A] == "padded")
    if A >= 2:
        assert float(q_tg.min()) == Q_TG_LOW < Q_MIN
        assert not bool((ref["qa_tg"] == Q_TG_LOW).any())
    # a row of q_tg holds distinct values: qa_tg names the greedy action
    if A >= 2:
        assert float(np.diff(np.sort(q_tg.astype(np.float64), 1), axis=1).min()) > 0
    v = ((1.0 + q_on.astype(np.float64)) - Q_MIN) * legal
    deep = deep_row(roles, A)
    e = ref["e"].reshape(-1)
    for r, role in enumerate(roles):
        if role == "padded":  # legal all zero, action 0: greedy 0, no error, no gradient
            assert legal[r].sum() == 0 and act[r] == 0 and ref["greedy"][r] == 0
            assert float(np.abs(q_on[r]).max()) > 0 or A == 1  # (the nets still produce Q-values there)
            assert r >= seq * batch or e[r] == 0
            continue
        assert r < seq * batch and legal[r, act[r]] == 1
        top = np.sort(v[r])[::-1]
        if role == "tie" and A >= 2:
            hi = np.flatnonzero(v[r] == top[0])
            assert len(hi) == 2 and ref["greedy"][r] == hi[0] and q_on[r, hi[0]] == q_on[r, hi[1]]
        elif A >= 2:
            assert top[0] - top[1] >= GRID or top[1] == 0, r  # (a single legal action: the rest are zeros)
            assert top[0] > 0
        if role == "illegal_best" and A >= 2:
            assert legal[r, int(q_on[r].argmax())] == 0 and ref["greedy"][r] != int(q_on[r].argmax())
        if role == "single_legal":
            assert legal[r].sum() == 1 and ref["greedy"][r] == act[r]
        if role == "act_last":
            assert act[r] == A - 1
        if role == "boot0_huge":
            assert inp["bootstrap"][r] == 0 and abs(float(ref["qa_tg"][r + n * batch])) >= 1e30
            assert abs(e[r]) <= 0.9
        if role.startswith("dyadic"):
            assert e[r] == {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[role], (r, e[r])
            assert float(inp["reward"][r]) * 64 == round(float(inp["reward"][r]) * 64) and inp["bootstrap"][r] == 1
        elif role.startswith("large"):
            assert abs(e[r]) >= 1.1 and np.sign(e[r]) == (1 if role == "large_pos" else -1), (r, e[r])
        elif role != "boot0_huge":
            assert abs(e[r]) <= 0.9, (r, e[r])
        if r == deep:  # only the true minimum keeps its legal actions ahead of the illegal column 0
            assert r * A >= 1025 and legal[r, 0] == 0 and float(q_on[r].max()) <= Q_DEEP + 3.0
            assert place < 1024 or float(flat[:1024].min()) > float(q_on[r].max()) + 1.0  # (element 1023 is inside)
    return ref


# ---- restated defects (tests/test_seq_loss_ref_cpu.py) --------------------------------------------------------------------------
DEFECTS = ("pad_mask_gt", "pad_mask_seq_len", "target_row_n_minus_1", "mean_over_seq_len", "priority_mask_dropped",
           "min_first_1024", "min_with_q_tg", "last_max", "argmax_ignores_legal", "one_over_num_legal", "value_in_column_A",
           "loss_mean_over_1024", "one_minus_eta_f32")


def loss_margins(inp, ref, defect):
    """what the GPU test's checks would see if the kernel computed seq_reference(defect=...): -> {check: margin}, a margin
    above 1 (or True) fails that check.  The exact checks: qa_tg (the greedy action) bit for bit, e on the dyadic rows,
    zeros of d_ha; the bounded ones in units of their derived bound, each continued from the DEFECTIVE e as the test
    continues from the kernel's own."""
    A, seq = inp["A"], inp["seq"]
    bad = seq_reference(defect=defect, **loss_args(inp))
    after = seq_reference(e=bad["e"], **loss_args(inp))
    tiny = 1e-300
    dyadic = np.array([role.startswith("dyadic") for role in row_roles(inp["batch"], seq, inp["burn"], inp["n"])[:seq * inp["batch"]]])
    out = {"qa_tg": not np.array_equal(bad["qa_tg"], ref["qa_tg"]),
           "e_dyadic": bool((bad["e"].reshape(-1)[dyadic] != ref["e"].reshape(-1)[dyadic]).any()),
           "loss_seq": float((np.abs(bad["loss_seq"] - after["loss_seq"]) /
                              np.maximum(_k(loss_seq_roundings(seq)) * after["loss_seq"], tiny)).max()),
           "e": float((np.abs(bad["e"] - ref["e"]) / np.maximum(e_bound(ref), tiny)).max()),
           "d_ha_zeros": bool((bad["d_ha"][:, A:31] != 0).any()) or bool((bad["d_ha"][:, :A][inp["legal"] == 0] != 0).any()),
           "d_ha": float((np.abs(bad["d_ha"] - after["d_ha"])[:, :A] / np.maximum(d_ha_bound(after), tiny)).max()),
           "d_v": float((np.abs(bad["d_ha"][:, 31] - after["dqa"]) / np.maximum(dqa_bound(after), tiny)).max()),
           "priority": float((np.abs(bad["priority"] - after["priority"]) /
                              np.maximum(_k(priority_roundings(seq)) * after["priority"], tiny)).max()),
           "loss": abs(bad["loss"] - after["loss"]) / max(_k(loss_roundings(seq)) * after["loss"], tiny)}
    # (exact differences where the bound is zero count as failures: a zero bound asks for equality)
    return out


def caught(margins):
    return [k for k, m in margins.items() if (m is True) or (m is not False and m > 1.0)]


# ---- the head backward -----------------------------------------------------------------------------------------------------------
HEAD_KEYS = ("d_o", "g_fc_a_w", "g_fc_a_b", "g_fc_v_w", "g_fc_v_b")
HEAD_ROWS = (1, 5, 33, 129, 1023, 1024, 1025, 2051)
HEAD_CASES = [(rows, A) for rows in HEAD_ROWS for A in (A_LIST if rows in (33, 1024) else (18,))]
SPLIT_ROWS, SPLIT_SLICES = 1024, 32  # csrc/learner_plan.h: kSeqHeadSplitRows, kSplitHeads


def head_shapes(rows, A):
    return {"d_o": (rows, 512), "g_fc_a_w": (A, 512), "g_fc_a_b": (A,), "g_fc_v_w": (1, 512), "g_fc_v_b": (1,)}


def _head_eval(A, d, o, aw, vw):
    dA, dV = d[:, :A], d[:, 31:32]
    return {"d_o": dA @ aw + dV @ vw, "g_fc_a_w": dA.t() @ o, "g_fc_a_b": dA.sum(0), "g_fc_v_w": dV.t() @ o,
            "g_fc_v_b": dV.sum(0)}


def _head_prep(A, d_ha, o, fc_a_w, fc_v_w, device):
    f = lambda x: torch.as_tensor(x).detach().to(device).to(torch.float64)
    return f(d_ha).reshape(-1, 32), f(o).reshape(-1, 512), f(fc_a_w).reshape(A, 512), f(fc_v_w).reshape(1, 512)


def head_reference(A, d_ha, o, fc_a_w, fc_v_w, device="cpu", defect=None):
    """-> {key: float64 tensor} for HEAD_KEYS.  defect (the weight gradients only): "wgrad_missing_last_row", or
    "wgrad_missing_slice": the last non-empty one of the 32 split-K slices of K chunks of 32 rows (gemm_lds: kslice =
    ceil(ceil(rows / 32) / 32) chunks per slice), which the learner runs from 1,024 rows"""
    d, o, aw, vw = _head_prep(A, d_ha, o, fc_a_w, fc_v_w, device)
    with torch.no_grad():
        out = _head_eval(A, d, o, aw, vw)
        keep = d.shape[0]
        if defect == "wgrad_missing_last_row":
            keep -= 1
        if defect == "wgrad_missing_slice":  # the last slice that holds rows
            chunks = -(-d.shape[0] // 32)
            kslice = -(-chunks // SPLIT_SLICES)
            keep = (-(-chunks // kslice) - 1) * kslice * 32
        if keep != d.shape[0]:
            part = _head_eval(A, d[:keep], o[:keep], aw, vw)
            out["g_fc_a_w"], out["g_fc_v_w"] = part["g_fc_a_w"], part["g_fc_v_w"]
        return out


def head_reference_abs(A, d_ha, o, fc_a_w, fc_v_w, device="cpu"):
    """per output element the sum of the absolute values of its terms: the scale of err_units"""
    d, o, aw, vw = _head_prep(A, d_ha, o, fc_a_w, fc_v_w, device)
    with torch.no_grad():
        return _head_eval(A, d.abs(), o.abs(), aw.abs(), vw.abs())


def head_n_terms(key, rows, A):
    """the a-priori bound in units of u * sum|terms|: a float32 sum of n products in any order is within n u sum|terms| of
    the exact one to first order (n - 1 additions and the product's own rounding): `rows` for the four gradients, A + 1 for
    d_o"""
    return float(A + 1 if key == "d_o" else rows)


# Exact data: d_ha = integers * 2^-6, weights = integers * 2^-4, o integers: every term of an output is a whole number of
# HEAD_UNIT[key] and every sum stays below 2^24 units, so float32 sums are exact in any order, tiling and split.
#   rows:  row r carries ONE non-zero entry of d_ha, +-2^-6 in column cols[r % (A + 1)] (cols = 0..A-1, 31), and o[r][u] =
#          2^p(r) where u % G == g(r), 0 elsewhere, with j = r // (A + 1), p = j % 24, g = j // 24: the rows behind one
#          element of a weight gradient carry DISTINCT powers of two 2^0 .. 2^23, so a dropped or doubled row or slice
#          changes it whatever else happens; a bias gradient is a signed count of its column's rows.
#   dense: small integers everywhere, columns A..30 of d_ha non-zero (they must not leak), o in 0..3.
E_D, E_W = 6, 4
HEAD_UNIT = {"d_o": 2.0 ** -(E_D + E_W), "g_fc_a_w": 2.0 ** -E_D, "g_fc_a_b": 2.0 ** -E_D, "g_fc_v_w": 2.0 ** -E_D,
             "g_fc_v_b": 2.0 ** -E_D}
HEAD_DATA_SETS = ("rows", "dense")


@functools.lru_cache(maxsize=2)
def head_exact_inputs(name, rows, A):
    rng = np.random.default_rng({"rows": 411, "dense": 422}[name] + 10 * rows + A)
    f = np.float32
    sign = lambda shape: rng.integers(0, 2, shape).astype(np.int64) * 2 - 1
    small = lambda shape: rng.integers(1, 4, shape).astype(np.int64)
    w = lambda shape: (small(shape) * sign(shape)).astype(f) * f(2.0 ** -E_W)
    if name == "rows":
        cols = list(range(A)) + [31]
        j = np.arange(rows) // len(cols)
        G = int(j.max()) // 24 + 1
        d = np.zeros((rows, 32), f)
        d[np.arange(rows), [cols[r % len(cols)] for r in range(rows)]] = sign(rows).astype(f) * f(2.0 ** -E_D)
        o = np.zeros((rows, 512), f)
        on = (np.arange(512)[None, :] % G) == (j // 24)[:, None]
        o[on] = np.broadcast_to((2.0 ** (j % 24)).astype(f)[:, None], (rows, 512))[on]
    else:
        d = (small((rows, 32)) * sign((rows, 32))).astype(f) * f(2.0 ** -E_D)
        o = rng.integers(0, 4, (rows, 512)).astype(f)
    return {"A": A, "d_ha": d, "o": o, "fc_a_w": w((A, 512)), "fc_v_w": w((1, 512))}


def head_exact_preconditions(name, inp, ref, ref_abs):
    """asserted on the inputs and the REFERENCE: whole numbers of units below 2^24, and for `rows` the distinct powers"""
    for key in HEAD_KEYS:
        total = float(ref_abs[key].max()) / HEAD_UNIT[key]
        assert total < 2 ** 24, "%s: sum|terms| of %s reaches %.0f units" % (name, key, total)
        val = ref[key] / HEAD_UNIT[key]
        assert bool((val == val.round()).all()), (name, key)
    if name == "rows":
        d, o = np.asarray(inp["d_ha"], np.float64), np.asarray(inp["o"], np.float64)
        assert bool(((d != 0).sum(1) == 1).all()) and bool(((o != 0).sum(1) >= 1).all())
        for k in list(range(inp["A"])) + [31]:
            sel = o[d[:, k] != 0]  # the rows behind row k of the weight gradient: per column u distinct powers of two
            for u in (0, 1, 255, 511):
                vals = sel[:, u][sel[:, u] != 0]
                assert len(set(vals.tolist())) == len(vals), (k, u)


@functools.lru_cache(maxsize=2)
def head_random_inputs(rows, A, seed=7):
    """d_ha with the loss kernel's structure: g_r * legal * ([k == a_r] - 1 / A) in columns < A, g_r in column 31, zeros in
    between, g_r = normal / rows with a fifth of the rows padded (all zero); o = o_gate * tanh(c) in (-1, 1); head weights of
    synth_lstm_params"""
    from synth import synth_lstm_params

    rng = np.random.default_rng(seed + 1000 * rows + A)
    p = synth_lstm_params(A, seed)
    g = (rng.standard_normal(rows) / rows).astype(np.float32)
    act = rng.integers(0, A, rows)
    legal = (rng.uniform(size=(rows, A)) < 0.7).astype(np.float32)
    legal[np.arange(rows), act] = 1
    padded = rng.uniform(size=rows) < 0.2
    g[padded], legal[padded] = 0, 0
    ind = np.zeros((rows, A), np.float32)
    ind[np.arange(rows), act] = 1
    d = np.zeros((rows, 32), np.float32)
    d[:, :A] = legal * (g[:, None] * (ind - np.float32(1.0 / A)))
    d[:, 31] = g
    o = (rng.uniform(0, 1, (rows, 512)) * np.tanh(rng.standard_normal((rows, 512)))).astype(np.float32)
    return {"A": A, "d_ha": d, "o": o, "fc_a_w": np.ascontiguousarray(p["fc_a.weight"]), "fc_v_w": np.ascontiguousarray(p["fc_v.weight"])}
