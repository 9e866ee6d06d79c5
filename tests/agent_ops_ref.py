"""Exact references of the actor-side ops of rela_amd/csrc/agent_ops.hip (act_kernel, td_kernel), in plain numpy: the
counter-based Philox4x32-10 of Salmon et al. (SC'11) written from the published algorithm, eps-greedy with the grouped
minimum of ApexAgent.greedy_act (pyrela/apex.py:48-65), the TD error and priority of pyrela/apex.py:30-45,68-78; the role
tables tests/test_agent_ops_exact_gpu.py runs, built by role; and one-line restatements of the defects those tables must
tell from the truth (tests/test_agent_ops_ref_cpu.py).  No torch, no GPU."""
import numpy as np

F = np.float32
MASK32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # multipliers
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # Weyl increments of the key


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------
def _philox4x32_10_words(c0, c1, c2, c3, k0, k1):
    """ten rounds on the full four-word counter (c0..c3) and two-word key, every word a uint64 array (or scalar) that holds
    32 bits.  One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, counter <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0);
    the key is bumped by the Weyl increments between rounds.  -> four uint32 arrays"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, np.uint64)) & MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = (np.atleast_1d(np.asarray(k, np.uint64)) & MASK32 for k in (k0, k1))
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _u64(x):
    """a Python int (any size, reduced modulo 2^64) or an array -> uint64 array"""
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) & 0xFFFFFFFFFFFFFFFF], np.uint64)
    return np.asarray(x, np.uint64)


def philox4x32_10(seed, ctr):
    """key = (seed lo, seed hi), counter = (ctr lo, ctr hi, 0, 0); `ctr` a uint64 array -> (r0, r1, r2, r3) uint32 arrays"""
    seed, ctr = _u64(seed), _u64(ctr)
    zero = np.zeros_like(ctr)
    return _philox4x32_10_words(ctr & MASK32, ctr >> np.uint64(32), zero, zero, seed & MASK32, seed >> np.uint64(32))


def counters(offset, n):
    """offset + row for n rows, modulo 2^64"""
    with np.errstate(over="ignore"):
        return _u64(offset) + np.arange(n, dtype=np.uint64)


def draws(seed, ctr):
    """-> (u, r1): the coin u = (r0 >> 8) * 2^-24 (torch.rand's 24-bit uniform, exact in float32) and the word of the pick"""
    r0, r1, _, _ = philox4x32_10(seed, ctr)
    return (r0 >> np.uint32(8)).astype(F) * F(2.0 ** -24), r1


def pick_of(word, nl):
    """(word * nl) >> 32: uniform on 0..nl-1 (0 where nl == 0)"""
    return ((word.astype(np.uint64) * np.asarray(nl, np.uint64)) >> np.uint64(32)).astype(np.int64)


def nth_legal(legal, pick):
    """index of the pick-th column with legal > 0 of every row (-1 where the row has no such column)"""
    on = np.asarray(legal) > 0
    order = np.cumsum(on, axis=1) - 1
    hit = on & (order == np.asarray(pick)[:, None])
    return np.where(hit.any(1), hit.argmax(1), -1)


# ---- the grouped minimum and the greedy rule ------------------------------------------------------------------------------
def group_bounds(n, group):
    g = group if group > 0 else n
    return [(r0, min(n, r0 + g)) for r0 in range(0, n, g)]


def launch_threads(n, group):
    """the workgroup size the launchers choose: 1,024 threads from groups of 512 rows, 256 below"""
    return 1024 if (group if group > 0 else n) >= 512 else 256


def _fmin(x):
    """float32 minimum that skips NaN, +inf over nothing (fminf from +inf)"""
    x = np.asarray(x, F).ravel()
    return F(np.fmin.reduce(np.concatenate([np.array([np.inf], F), x])))


def group_min(q, group, defect=None):
    """[n] the minimum every row's greedy rule subtracts: over the row's group of `group` consecutive rows (0: the whole
    batch; the last group may be short).  `defect`: see MIN_DEFECTS."""
    n, A = q.shape
    out = np.empty(n, F)
    prev = F(np.inf)
    for r0, r1 in group_bounds(n, group):
        lo, hi = r0 * A, r1 * A
        if defect == "min_reads_next_row":
            hi = min(n, r1 + 1) * A
        elif defect == "min_misses_last_row":
            hi = (r1 - 1) * A
        elif defect == "min_misses_last_two_rows":
            hi = max(r0, r1 - 2) * A
        elif defect == "min_misses_last_element":
            hi = r1 * A - 1
        elif defect == "min_single_pass":
            hi = min(hi, lo + launch_threads(n, group))
        m = _fmin(q.reshape(-1)[lo:hi])
        if defect == "min_carried_over":
            m = prev = min(m, prev)
        out[r0:r1] = m
    return out


def greedy_ref(q, legal, group, defect=None):
    """first maximal index of ((1 + q) - qmin) * legal, every operation rounded to float32, compared with a strict > from
    -inf (a NaN entry never wins; a row of nothing but NaN gives 0)"""
    q, legal = np.asarray(q, F), np.asarray(legal, F)
    qmin = group_min(q, group, defect)
    with np.errstate(invalid="ignore", over="ignore"):
        lq = ((F(1.0) + q) - qmin[:, None]) * legal
    assert lq.dtype == F
    best, bv = np.zeros(q.shape[0], np.int64), np.full(q.shape[0], -np.inf, F)
    for j in range(q.shape[1]):
        better = lq[:, j] > bv
        best[better], bv[better] = j, lq[better, j]
    return best


# ---- eps-greedy -----------------------------------------------------------------------------------------------------------
def eps_select(greedy, legal, eps, seed, ctr, defect=None):
    """the random branch on top of given greedy actions, row i drawing at counter ctr[i]: only where eps > 0 (0, negative
    and NaN consult no draw), random iff u < eps, then the pick-th of the nl legal columns, pick = (r1 * nl) >> 32; a row
    without a legal column stays greedy.  -> dict(action, u, pick, nl, random); u and pick are given for EVERY row, as the
    row would draw them, so that tests can address rows by what they would do."""
    legal, eps = np.asarray(legal, F), np.asarray(eps, F).reshape(-1)
    u, r1 = draws(seed, ctr)
    nl = (legal > 0).sum(1)
    pick = pick_of(r1, nl)
    with np.errstate(invalid="ignore"):
        coin = (u <= eps) if defect == "coin_le" else (u < eps)
        rand = (eps > 0) & coin & (nl > 0)
    take = pick
    if defect == "pick_from_coin_word":
        take = pick_of(philox4x32_10(seed, ctr)[0], nl)
    elif defect == "pick_over_A":  # the walk over the legal columns ends without a hit: the row stays greedy
        take = pick_of(r1, np.full_like(nl, legal.shape[1]))
    chosen = nth_legal(legal, take)
    action = np.where(rand & (chosen >= 0), chosen, greedy)
    return dict(action=action.astype(np.int64), u=u, pick=pick, nl=nl, random=rand)


def eps_greedy_ref(q, legal, eps, group, seed, offset, defect=None):
    """act_kernel: row i of the call draws at counter offset + i.  -> dict(action, greedy, u, pick, nl, random)"""
    n = np.asarray(q).shape[0]
    greedy = greedy_ref(q, legal, group, defect)
    ctr = counters(offset, n)
    if defect == "ctr_ignores_offset":  # what a shard that never advances its tick count amounts to
        ctr = counters(0, n)
    elif defect == "ctr_row_in_group":
        ctr = np.concatenate([counters(offset, r1 - r0) for r0, r1 in group_bounds(n, group)])
    out = eps_select(greedy, legal, eps, seed, ctr, defect)
    out["greedy"] = greedy
    return out


# ---- TD error and priority ------------------------------------------------------------------------------------------------
def td_ref(q, q_next_online, q_next_target, next_legal, action, reward, bootstrap, gamma_n, group, vr_eps=0.0, defect=None):
    """td_kernel: next action greedy over q_next_online with the grouped minimum, target = reward + (bootstrap * gamma_n) *
    q_next_target[next action], un-fused float32; error = target - q[action], priority = |error|.  vr_eps > 0: the target is
    h(reward + (bootstrap * gamma_n) * h_inv(q_next_target[..])) through the host build of csrc/value_rescale.h
    (tests/value_rescale_util.py).  -> (error, priority, next action)"""
    q, qnt = np.asarray(q, F), np.asarray(q_next_target, F)
    rows = np.arange(q.shape[0])
    na = greedy_ref(q_next_online, next_legal, group, defect)
    qa, bq = q[rows, np.asarray(action)], qnt[rows, na]
    g = np.asarray(bootstrap, F) * F(gamma_n)
    if vr_eps > 0:
        from value_rescale_util import host_h_hinv

        _, bq = host_h_hinv(bq, vr_eps)
        tgt, _ = host_h_hinv(np.asarray(reward, F) + g * bq, vr_eps)
    else:
        tgt = np.asarray(reward, F) + g * bq
    err = tgt - qa
    assert err.dtype == F
    return err, np.abs(err), na


# ---- the role tables ------------------------------------------------------------------------------------------------------
# (n, group_rows, A): the smallest shapes that reach each path of the launchers and kernels
SHAPES = [(1, 0, 1),         # single row, single column
          (19, 8, 6),        # 256 threads, ragged last group of 3
          (40, 1, 18),       # every row its own minimum
          (603, 300, 18),    # 256 threads, two passes of the row loop, ragged
          (1027, 512, 6),    # 1,024 threads, the threshold itself, ragged
          (1030, 1025, 18),  # 1,024 threads, two passes
          (700, 0, 18)]      # the whole batch as one group: 256 threads, three passes
SEED, OFFSET = 0x5EED0123456789AB, 3 * (1 << 32) + 977  # of the role tables: both halves of key and counter in use
LEAK_VALUE = F(-2.0 ** 26)
HIGH = F(2.0 ** 28)  # a value that wins its row's greedy rule in every group

# the roles a free row can take, dealt in this order: (name, eps kind, legal kind, q kind)
ROW_ROLES = [
    ("tie", "zero", "all", "tie"),                   # two equal maxima: the first wins
    ("nan_column", "negative", "all", "nan"),        # a NaN column is never chosen; negative eps: greedy, no draw
    ("eps_equals_u", "u", "all", "high_off_pick"),   # eps == u exactly: greedy
    ("one_legal_first", "one", "first", None),
    ("one_legal_last", "one", "last", None),
    ("none_legal", "one", "none", None),             # stays greedy: action 0
    ("eps_nan", "nan", "all", None),                 # greedy, no draw
    ("eps_tiny", "2^-24", "partial", "high_off_pick"),  # random only where r0 >> 8 == 0
    # (the rows that draw and have a choice come last)
    ("eps_next_after_u", "u_next", "all", "high_off_pick"),  # the next float32 above u: random
    ("eps_one_partial", "one", "partial", "high_off_pick"),  # always random, 2 <= nl < A
    ("eps_one_all", "one", "all", "high_off_pick"),
    ("eps_above_one", "1.5", "all", "high_off_pick"),
]
ROLE_NAMES = [r[0] for r in ROW_ROLES] + ["single_column", "leak", "leak_source", "miss_last_row", "miss_other_row",
                                          "miss_last_element", "min_last_element"]


def role_cases(n, group, A, seed=SEED, offset=OFFSET):
    """The inputs of one shape: q [n, A] (also td's q_next_online), legal [n, A] (also td's next_legal), eps [n], the
    other inputs of td, and roles: name -> rows.

    Groups alternate.  Even groups hold values around 0; an odd group's first row holds -2^26 in its first element, right
    behind the last element of the group before it (leak_source; leak: the rows of that group which a minimum reaching
    into the source moves: every 1 + q - qmin collapses to one value and the first legal column wins).  In every group the
    minimum sits in the last element of the last row (min_last_element).  In an even group that element is the row's only
    legal one (miss_last_element, miss_last_row: a minimum without it leaves the entry negative, and the illegal column 0
    wins); in an odd group, where 1 + q - qmin of the minimum itself rounds to 0, the last row's legal entries lie far below
    the rest of the group instead (miss_last_row), as do, less far, those of the row before the last in every group
    (miss_other_row: a minimum that skips both rows).  The deep entries rise with the column, so that the rows tell a
    collapsed group (column 1) from a true one (column A - 2) too.  All other rows are dealt ROW_ROLES in turn."""
    assert A == 1 or A >= 3  # (two columns cannot hold a tie beside a third value, nor a partial mask)
    rng = np.random.default_rng(1000 * n + 10 * group + A)
    q = rng.normal(0, 1, (n, A)).astype(F)
    legal = np.ones((n, A), F)
    eps = np.zeros(n, F)
    roles = {k: [] for k in ROLE_NAMES}
    u, r1 = draws(seed, counters(offset, n))
    bounds = group_bounds(n, group)
    free = []
    for gi, (r0, r1g) in enumerate(bounds):
        m, odd = r1g - r0, gi % 2 == 1
        # deep rows: below what the rest of the group reaches down to.  Even groups: steps of 1/64 around 1 + q = -20, so
        # that all of a row rounds to one value beside 2^26 and beyond; odd groups: steps that stay apart beside 2^29
        deep, unit, step = (F(-2.0 ** 26), F(2.0 ** 22), F(2.0 ** 22)) if odd else (F(-1.0), F(1.0), F(1.0 / 64))
        special = set()

        def deep_row(row, base):  # columns 1 .. A-2 legal and far below the group, the highest of them last
            legal[row, 0] = legal[row, A - 1] = 0
            q[row, 1:A - 1] = deep - unit * F(base) - step * np.arange(A - 2, 0, -1, dtype=F)
            special.add(row)

        if odd:
            q[r0, 0] = LEAK_VALUE
            roles["leak_source"].append(r0)
            special.add(r0)
        last = r1g - 1
        if m >= 2 and A >= 2 and not odd:
            legal[last] = 0
            legal[last, A - 1] = 1
            special.add(last)
            roles["miss_last_element"].append(last)
            roles["miss_last_row"].append(last)
        elif m >= 2 and A >= 3:
            deep_row(last, 50)
            roles["miss_last_row"].append(last)
        if m >= 3 and A >= 3:
            deep_row(last - 1, 20)
            roles["miss_other_row"].append(last - 1)
        free += [r for r in range(r0, r1g) if r not in special]
        if m >= 2:  # (a group of one row: its minimum is where it falls)
            q[last, A - 1] = F(-2.0 ** 29) if odd else F(-1000.0)
            roles["min_last_element"].append(last)
    # rows of even groups first, so that the roles whose q matters (tie, nan_column) land where values are not collapsed
    even_rows = {r for gi, (r0, r1g) in enumerate(bounds) if gi % 2 == 0 for r in range(r0, r1g)}
    # ... and the rows of odd groups take the list from its end: the rows that draw and have a choice, in every group
    dealt = [(r, k) for k, r in enumerate(r for r in free if r in even_rows)]
    dealt += [(r, len(ROW_ROLES) - 1 - k) for k, r in enumerate(r for r in free if r not in even_rows)]
    for row, k in dealt:
        name, eps_kind, legal_kind, q_kind = ROW_ROLES[k % len(ROW_ROLES)]
        if A == 1:  # one column: always legal, nothing to tie with, and every draw picks it
            name, eps_kind, legal_kind, q_kind = "single_column", "one", "all", None
        if legal_kind == "partial":
            on = rng.uniform(size=A) < 0.5
            on[rng.choice(A, 3, replace=False)] = [True, True, False]  # at least two legal columns, one illegal
            legal[row] = on
        elif legal_kind in ("first", "last", "none"):
            legal[row] = 0
            if legal_kind != "none":
                legal[row, 0 if legal_kind == "first" else A - 1] = 1
        keep = q[row, A - 1] if row in roles["min_last_element"] else None
        if q_kind == "tie" and A >= 3:
            q[row, 1] = q[row, A - 2 if A > 3 else 2] = HIGH
        elif q_kind == "nan" and A >= 2:
            q[row, 1] = np.nan
        elif q_kind == "high_off_pick" and A >= 2:  # greedy differs from what the row's draw would pick
            nl = int((legal[row] > 0).sum())
            picked = int(nth_legal(legal[row:row + 1], pick_of(r1[row:row + 1], nl))[0])
            others = [j for j in np.flatnonzero(legal[row] > 0) if j != picked and not (keep is not None and j == A - 1)]
            if others:
                q[row, others[0]] = HIGH
        eps[row] = {"zero": F(0), "negative": F(-0.25), "nan": F(np.nan), "one": F(1), "1.5": F(1.5),
                    "2^-24": F(2.0 ** -24), "u": u[row], "u_next": np.nextafter(u[row], F(1))}[eps_kind]
        roles[name].append(row)
    ref = greedy_ref(q, legal, group)
    for gi, (r0, r1g) in enumerate(bounds[:-1]):  # rows a leak from the group behind them would move
        if gi % 2 == 0:
            on = legal[r0:r1g] > 0
            first_legal = np.where(on.any(1), on.argmax(1), 0)
            for r in range(r0, r1g):  # ... whose legal entries all round to ONE value beside 2^26
                beside = ((F(1.0) + q[r]) - LEAK_VALUE)[on[r - r0] & ~np.isnan(q[r])]
                if ref[r] != first_legal[r - r0] and len(beside) and (beside == beside[0]).all():
                    roles["leak"].append(r)
    rng2 = np.random.default_rng(7000 + n)
    td = dict(q=rng2.normal(0, 1, (n, A)).astype(F), qnt=rng2.normal(0, 1, (n, A)).astype(F),
              action=rng2.integers(0, A, n).astype(np.int64), reward=rng2.integers(-1, 2, n).astype(F),
              bootstrap=(rng2.uniform(size=n) < 0.8).astype(F), gamma_n=F(0.997 ** 3))
    td["bootstrap"][roles["miss_last_row"] + roles["miss_other_row"]] = 1  # their next action reaches the priority
    for a in (q, legal, eps, *td.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(n=n, group=group, A=A, q=q, legal=legal, eps=eps, seed=seed, offset=offset, td=td,
                roles={k: np.array(v, np.int64) for k, v in roles.items()})


# ---- restated defects -----------------------------------------------------------------------------------------------------
MIN_DEFECTS = ("min_reads_next_row",        # the minimum of a group reads into the first row of the next one
               "min_carried_over",          # ... or is not reset between groups
               "min_misses_last_row", "min_misses_last_two_rows",
               "min_single_pass",           # only the first blockDim.x elements of the group
               "min_misses_last_element")
DEFECTS = ("ctr_ignores_offset", "ctr_row_in_group", "pick_from_coin_word", "coin_le", "pick_over_A") + MIN_DEFECTS


def run_case(case, defect=None):
    """everything tests/test_agent_ops_exact_gpu.py compares at one shape: the actions under the table's eps, the greedy
    column (the same call with eps = 0), td's error and priority"""
    act = eps_greedy_ref(case["q"], case["legal"], case["eps"], case["group"], case["seed"], case["offset"], defect)
    td = case["td"]
    err, prio, _ = td_ref(td["q"], case["q"], td["qnt"], case["legal"], td["action"], td["reward"], td["bootstrap"],
                          td["gamma_n"], case["group"], defect=defect)
    return dict(action=act["action"], greedy=act["greedy"], td=err, prio=prio, draw=act)


def rows_that_differ(a, b):
    """rows on which two run_case results differ in anything the GPU test compares (floats by their bits)"""
    bad = (a["action"] != b["action"]) | (a["greedy"] != b["greedy"])
    for k in ("td", "prio"):
        bad |= a[k].view(np.uint32) != b[k].view(np.uint32)
    return np.flatnonzero(bad)
