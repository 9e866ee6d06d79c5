"""tests/agent_ops_ref.py on the CPU: its Philox4x32-10 gives Random123's published known answers and equals a plain-Python
restatement; its greedy rule equals the C oracle's, grouped and not; the draw scheme is uniform, so that the GPU test need
not be statistical; the role tables of tests/test_agent_ops_exact_gpu.py hold every role at every shape and the reference
alone behaves as each role says; and one-line restatements of the defects the tables exist for are told from the truth on a
tagged row -- or are named here as invisible, with the reason."""
import ctypes as C
import functools

import numpy as np
import pytest

import agent_ops_ref as R

F = np.float32
SHAPE_IDS = ["n%d-group%d-A%d" % s for s in R.SHAPES]


# ---- Philox ---------------------------------------------------------------------------------------------------------------
def philox_python(ctr, key):
    """Philox4x32-10 on Python integers, from the paper: ctr four words, key two words -> four words"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KNOWN_ANSWERS = [  # Random123 kat_vectors, philox4x32 10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    assert tuple(philox_python(ctr, key)) == want
    got = R._philox4x32_10_words(*ctr, *key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_vectorised_equals_plain_python():
    rng = np.random.default_rng(1)
    seeds = [0, 1, 1 << 32, (1 << 64) - 1, 11, R.SEED]
    ctr = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1] + [int(x) for x in rng.integers(0, 1 << 63, 40)], np.uint64)
    for seed in seeds:
        got = R.philox4x32_10(seed, ctr)
        for i, c in enumerate(int(x) for x in ctr):
            want = philox_python((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
            assert [int(w[i]) for w in got] == want, (seed, c)


def test_seed_0_counter_0_coin_and_picks():
    u, r1 = R.draws(0, R.counters(0, 1))
    assert float(u[0]) == 0.3990464210510254 and u.dtype == F
    assert [int(R.pick_of(r1, nl)[0]) for nl in (1, 6, 12, 18)] == [0, 5, 10, 15]
    assert int(R.counters((1 << 64) - 1, 2)[1]) == 0  # the counter wraps modulo 2^64


def test_draw_scheme_is_uniform():
    """65,536 consecutive counters, nl = 12: every bin of the pick within five binomial standard deviations of n / 12, the
    fraction of u < 0.5 within five of one half.  (A seed that fails is a finding about the scheme, not a reason to pick
    another.)"""
    n, nl = 65536, 12
    u, r1 = R.draws(R.SEED, R.counters(0, n))
    hist = np.bincount(R.pick_of(r1, nl), minlength=nl)
    assert hist.sum() == n and len(hist) == nl
    sd = np.sqrt(n * (1 / nl) * (1 - 1 / nl))
    assert np.abs(hist - n / nl).max() <= 5 * sd, (hist, sd)
    assert abs(float((u < 0.5).mean()) - 0.5) <= 5 * 0.5 / np.sqrt(n)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0


# ---- the greedy rule equals the oracle's ------------------------------------------------------------------------------------
def oracle_greedy(q, legal):
    from oracle_lib import load

    lib = load()
    lib.oracle_greedy.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    q, legal = np.ascontiguousarray(q, F), np.ascontiguousarray(legal, F)
    out = np.zeros(q.shape[0], np.int64)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    lib.oracle_greedy(q.shape[0], q.shape[1], fp(q), fp(legal), out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out


@functools.lru_cache(maxsize=None)
def case_of(shape):
    return R.role_cases(*shape)


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_greedy_reference_equals_the_oracle(shape):
    """on the role table (ties, a NaN column, illegal columns, the values of the leak and miss rows) and on plain random data:
    as one group against oracle_greedy, grouped against oracle_greedy applied group by group"""
    n, group, A = shape
    case = case_of(shape)
    rng = np.random.default_rng(n)
    plain = (rng.normal(0, 1, (n, A)).astype(F), (rng.uniform(size=(n, A)) < 0.7).astype(F))
    for q, legal in ((case["q"], case["legal"]), plain):
        assert np.array_equal(R.greedy_ref(q, legal, 0), oracle_greedy(q, legal))
        by_group = np.concatenate([oracle_greedy(q[r0:r1], legal[r0:r1]) for r0, r1 in R.group_bounds(n, group)])
        assert np.array_equal(R.greedy_ref(q, legal, group), by_group)


def test_td_reference_equals_the_value_rescale_restatement():
    """td_ref with and without value rescaling, group by group, against td_priority_f32 of tests/value_rescale_util.py"""
    from value_rescale_util import EPS, td_priority_f32

    case = case_of((19, 8, 6))
    td = case["td"]
    qno = np.where(np.isnan(case["q"]), F(0.25), case["q"])  # (that restatement's numpy min and argmax let a NaN through)
    for vr in (0.0, EPS):
        _, prio, _ = R.td_ref(td["q"], qno, td["qnt"], case["legal"], td["action"], td["reward"], td["bootstrap"],
                              td["gamma_n"], 8, vr_eps=vr)
        for r0, r1 in R.group_bounds(19, 8):
            want = td_priority_f32(td["q"][r0:r1], qno[r0:r1], td["qnt"][r0:r1], case["legal"][r0:r1],
                                   td["action"][r0:r1], td["reward"][r0:r1], td["bootstrap"][r0:r1], td["gamma_n"], vr)
            assert np.array_equal(prio[r0:r1].view(np.uint32), np.asarray(want, F).view(np.uint32)), (vr, r0)


# ---- the role tables hold their roles -----------------------------------------------------------------------------------------
ALL_ROLES = set(R.ROLE_NAMES)
ONE_GROUP = {"leak", "leak_source"}  # nothing behind the only group
TOO_SMALL = {
    (1, 0, 1): ALL_ROLES - {"single_column"},       # one element: it is the action, whatever is drawn
    # one row per group: no row beside the minimum's (a minimum without that row is +inf here, and shows on most rows)
    (40, 1, 18): {"miss_last_row", "miss_other_row", "miss_last_element", "min_last_element", "single_column"},
    (700, 0, 18): ONE_GROUP | {"single_column"},
}


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_role_tables_hold_every_role_and_the_reference_behaves_as_the_role_says(shape):
    n, group, A = shape
    case = case_of(shape)
    roles, q, legal, eps = case["roles"], case["q"], case["legal"], case["eps"]
    present = {k for k, v in roles.items() if len(v)}
    assert ALL_ROLES - present == TOO_SMALL.get(shape, {"single_column"})
    tagged = np.concatenate([v for k, v in roles.items() if k not in ("leak", "min_last_element", "miss_last_element")])
    assert sorted(tagged.tolist()) == list(range(n))  # every row has exactly one role of its own
    ref = R.run_case(case)
    d = ref["draw"]
    act, greedy, u, rand = ref["action"], ref["greedy"], d["u"], d["random"]
    picked = R.nth_legal(legal, d["pick"])  # what the row's draw would choose
    assert (u > 0).all()  # no row has r0 >> 8 == 0: eps = 2^-24 is never random here
    assert (legal[np.arange(n), act] > 0).all() or len(roles["none_legal"])
    g = lambda name: roles[name]
    # greedy rows, with their reasons
    for name in ("tie", "eps_equals_u", "nan_column", "eps_nan", "eps_tiny", "none_legal"):
        assert not rand[g(name)].any() and np.array_equal(act[g(name)], greedy[g(name)]), name
    if A >= 3:
        rows = g("tie")
        assert (greedy[rows] == 1).all() and (q[rows, 1] == q[rows, A - 2 if A > 3 else 2]).all() and (q[rows, 1] == R.HIGH).all()
        assert (greedy[g("miss_other_row")] == A - 2).all()
        only_last = np.isin(g("miss_last_row"), g("miss_last_element"))  # (even groups: the minimum is the only legal entry)
        assert np.array_equal(greedy[g("miss_last_row")], np.where(only_last, A - 1, A - 2))
    if A >= 2:
        assert np.isnan(q[g("nan_column"), 1]).all() and (act[g("nan_column")] != 1).all() and (eps[g("nan_column")] < 0).all()
        assert np.isnan(eps[g("eps_nan")]).all()
        rows = g("eps_equals_u")
        assert (eps[rows] == u[rows]).all() and (picked[rows] != greedy[rows]).all()  # u <= eps would show
        rows = g("eps_next_after_u")
        assert (eps[rows] == np.nextafter(u[rows], F(1))).all() and rand[rows].all()
        assert np.array_equal(act[rows], picked[rows]) and (act[rows] != greedy[rows]).all()
        assert (eps[g("eps_tiny")] == F(2.0 ** -24)).all() and (picked[g("eps_tiny")] != greedy[g("eps_tiny")]).all()
        # random rows: the pick-th legal column
        for name in ("eps_one_partial", "eps_one_all", "eps_above_one", "one_legal_first", "one_legal_last"):
            assert rand[g(name)].all() and np.array_equal(act[g(name)], picked[g(name)]), name
        assert (eps[g("eps_above_one")] == 1.5).all()
        nl = d["nl"]
        assert ((nl[g("eps_one_partial")] > 0) & (nl[g("eps_one_partial")] < A)).all() and (nl[g("eps_one_all")] == A).all()
        assert (act[g("one_legal_first")] == 0).all() and (nl[g("one_legal_first")] == 1).all()
        assert (act[g("one_legal_last")] == A - 1).all() and (nl[g("one_legal_last")] == 1).all()
        assert (nl[g("none_legal")] == 0).all() and (act[g("none_legal")] == 0).all() and (eps[g("none_legal")] == 1).all()
    else:
        assert (act == 0).all() and rand[g("single_column")].all()
    # the minimum of every group is the last element of its last row
    qmin = R.group_min(q, group)
    for r0, r1 in R.group_bounds(n, group):
        if r1 - r0 >= 2:
            assert r1 - 1 in g("min_last_element") and q[r1 - 1, A - 1] == qmin[r0]
            assert (q[r0:r1].reshape(-1)[:-1][~np.isnan(q[r0:r1].reshape(-1)[:-1])] > qmin[r0]).all()
    # leak: the first element behind an even group is -2^26, and the rows tagged leak are those it would move to the first
    # legal column; miss: without the last row (the last two) the illegal column 0 wins
    for r in g("leak_source"):
        assert q[r, 0] == R.LEAK_VALUE and q[r, 0] == -2.0 ** 26
    leaked = R.greedy_ref(q, legal, group, "min_reads_next_row")
    assert (leaked[g("leak")] != greedy[g("leak")]).all()
    if len(g("leak")):
        first_legal = (legal[g("leak")] > 0).argmax(1)
        assert np.array_equal(leaked[g("leak")], first_legal)
    assert (R.greedy_ref(q, legal, group, "min_misses_last_row")[g("miss_last_row")] == 0).all()
    assert (R.greedy_ref(q, legal, group, "min_misses_last_element")[g("miss_last_element")] == 0).all()
    assert np.isin(g("miss_last_element"), g("min_last_element")).all()
    collapsed = R.greedy_ref(q, legal, group, "min_carried_over")[g("miss_other_row")]  # a collapsed group: column 1
    assert set(collapsed.tolist()) <= {1, A - 2} and (len(R.group_bounds(n, group)) < 3 or group == 1 or (collapsed == 1).any())
    assert (R.greedy_ref(q, legal, group, "min_misses_last_two_rows")[g("miss_other_row")] == 0).all()


# ---- the restated defects -------------------------------------------------------------------------------------------------------
def applies(defect, shape):
    """must the tables of this shape tell the restated defect from the truth?"""
    n, group, A = shape
    groups = len(R.group_bounds(n, group))
    elements = (group if group > 0 else n) * A
    return {
        # a counter that does not advance per tick: at the level of one call, an offset that is not used
        "ctr_ignores_offset": A >= 2,
        "ctr_row_in_group": A >= 2 and groups > 1,
        "pick_from_coin_word": A >= 2,
        "coin_le": A >= 2,
        "pick_over_A": A >= 2,
        "min_reads_next_row": groups > 1,
        # an even group behind an odd one: two groups are not enough (the second one holds the smaller minimum anyway)
        "min_carried_over": groups > 2,
        "min_misses_last_row": A >= 2,
        "min_misses_last_two_rows": A >= 2,
        "min_single_pass": elements > R.launch_threads(n, group),
        # one element: visible only because the tables make the minimum the ONLY legal entry of its row (below)
        "min_misses_last_element": A >= 2 and group != 1,
    }[defect]


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_restated_defects_show_on_a_tagged_row(shape, record_property):
    case = case_of(shape)
    truth = R.run_case(case)
    assert len(R.rows_that_differ(truth, R.run_case(case))) == 0
    for defect in R.DEFECTS:
        rows = R.rows_that_differ(truth, R.run_case(case, defect))
        record_property(defect, int(len(rows)))
        assert bool(len(rows)) == applies(defect, shape), (defect, rows[:8])


def test_a_missed_element_is_invisible_unless_it_is_the_only_legal_entry_of_its_row():
    """INVISIBLE, and not by accident of the data: a minimum that misses ONE element returns the next smallest one.  On
    every other element 1 + q - min stays >= 1 where it was >= 1 and the order within a row is what it was; only the
    missed element itself can fall below 0, and that moves an action only where no other legal entry is there to win.
    With a second legal entry in the minimum's row the defect changes nothing, at every shape -- which is why the tables
    make the minimum the only legal entry of its row, and why a minimum that misses any OTHER single element cannot be seen
    at all (it returns the same value)."""
    for shape in R.SHAPES:
        case = case_of(shape)
        n, group, A = shape
        legal = case["legal"].copy()
        for r in case["roles"]["min_last_element"]:
            if A >= 2 and (legal[r] > 0).sum() == 1 and legal[r, A - 1] > 0:
                legal[r, 0] = 1
        assert np.array_equal(R.greedy_ref(case["q"], legal, group, "min_misses_last_element"), R.greedy_ref(case["q"], legal, group))


def test_every_visible_defect_shows_in_the_actions_or_the_priorities_it_belongs_to():
    """the draw defects show in the actions under the table's eps and nowhere else; the minimum's show in the greedy column
    and in td's outputs (through the next action)"""
    case = case_of((603, 300, 18))
    truth = R.run_case(case)
    for defect in R.DEFECTS:
        bad = R.run_case(case, defect)
        if defect in R.MIN_DEFECTS:
            if applies(defect, (603, 300, 18)):
                assert (bad["greedy"] != truth["greedy"]).any() and (bad["prio"].view(np.uint32) != truth["prio"].view(np.uint32)).any()
        else:
            assert np.array_equal(bad["greedy"], truth["greedy"]) and np.array_equal(bad["td"].view(np.uint32), truth["td"].view(np.uint32))
            assert (bad["action"] != truth["action"]).any(), defect
