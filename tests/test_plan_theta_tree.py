"""The plan's theta-tree mode (include/qe_plan.h: qe_plan_run_text_theta_tree) on CPU: the compiled
plan of libqeplan.so over the numpy engine of tests/plan_engine_tree.py, against theta-tree truth
(tests/tree_truth.py, itself checked here against a brute-force nested-loop evaluator) -- chains,
stars and trees of column < / > column links, which theta mode refuses, and the 68 corpus cases
with such a predicate, none of which is refused any more."""
import numpy as np
import pytest
import torch.multiprocessing as mp

import plan_engine as pe
import plan_engine_tree as petr
import rel_truth as rt
import test_plan_theta as tpt
import theta_truth as tt
import tree_truth as trt

QE_EINVAL, QE_ETOOBIG, QE_ENOTSUP = -1, -5, -6

# hand-written shapes on test_plan_theta's small relations (40, 23 and 9 rows, values in [0, 8)):
# (query, what it exercises); every cross product stays below 10^7 tuples
HAND = [
    ("0 1 2|0.0<1.0&1.1<2.1|0.1 1.2 2.0", "a chain of 3, every component selected"),
    ("0 1 2|0.0<1.0&1.1<2.1|0.1", "a chain of 3, selected at a leaf only"),
    ("0 1 2|0.0<1.0&1.1<2.1|1.2", "a chain of 3, selected in the middle only"),
    ("0 1 2|0.0<1.0&1.1<2.1|0.1 2.2", "a chain of 3, selected at both ends"),
    ("0 1 2|0.0>1.0&1.1>2.1|0.1 2.2", "a chain of >"),
    ("0 1 2|1.0>0.0&2.1>1.1|0.1 2.0", "a chain whose predicates name the later binding first"),
    ("0 1 2 0|0.0<1.0&1.1>2.1&2.2<3.2|0.1 3.0", "a chain of 4, mixed < and >"),
    ("0 1 2 0|0.0<1.0&1.1>2.1&2.2<3.2|1.2 2.0", "a chain of 4, selected at its inner components"),
    ("1 0 2 2|0.0<1.0&0.1>2.1&0.2<3.2|1.1 2.0 3.1 0.2", "a star: a centre keyed on three columns, 3 leaves"),
    ("1 0 2 2|0.0<1.0&0.1>2.1&0.2<3.2|0.0", "a star selected at its centre only"),
    ("1 0 2 2|0.0<1.0&0.1>2.1&0.2<3.2|3.0", "a star selected at one leaf only"),
    ("0 1 2 2|0.0=1.0&0.1<2.1&1.2>3.2|0.2 1.1 2.0 3.0", "a joined centre keyed on two of its bindings"),
    ("0 1 2 2|0.0<1.0&1.1<2.1|0.1 3.2", "a chain next to an unlinked component"),
    ("2 2 2 2 1|0.0<1.0&1.1<2.1&3.0>4.0|0.1 2.2 3.1 4.2", "two trees in one query"),
    ("2 2 2 2 1|0.0<1.0&1.1<2.1&3.0>4.0|3.1", "two trees, one of them read by no select"),
    ("0 0 0|0.0<1.0&1.1<2.1|0.2 2.2", "a relation linked with itself twice"),
    ("0 1 2|0.0<1.0&1.1<2.1&0.2>3&1.0<6|0.1 1.1 2.1", "filters on a chain's components"),
    ("0 1 2 1|0.0<1.0&1.1<2.1&1.2=3.2&1.0>3.0|0.1 3.1 2.0", "a selection inside a chain's middle component"),
    ("0 1|0.0<1.0|0.1 1.1", "a tree of one edge: theta mode's link"),
    ("0 1 2|0.0<1.0&1.1<2.1&2.2>100|0.1", "a filter that empties a leaf: NULL"),
    ("0 1 2|0.0<1.0&1.1<2.1&2.1<1|0.1 1.1", "no tuple satisfies the chain: NULL"),
]
NULLS = 2                                                # lines of the table that are all NULL
BANDS = tpt.REFUSED[2:]
CYCLE = "0 1 2|0.0<1.0&1.1<2.1&2.2<0.2|0.1"
FORMERLY_REFUSED = {"fuzz_a": 1011812013687, "fuzz_c": 2315017298}   # the issue's pair counts


def _run_world(rels, queries, world, opts=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = pe.free_port()
    procs = [ctx.Process(target=petr.worker, args=(r, world, port, rels, queries, q, opts)) for r in range(world)]
    for p in procs:
        p.start()
    res = None
    try:
        while res is None:                               # (a rank that dies never reports: notice its exit)
            try:
                res = q.get(timeout=0.2)
            except tpt.queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a rank exited with {dead} before rank 0 reported"
                if all(p.exitcode == 0 for p in procs):
                    res = q.get(timeout=5)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(timeout=10)
    return res


def _engine(rels, optional="all", **kw):
    on = optional == "all"
    return petr.NumpyPlanEngineTree(rels, 0, 1, fused_scan=on, join_carry=on, join_sums=on, values=on, join_agg=on,
                                    key_carry=on, **kw)


def test_truth_is_the_nested_loops():
    rels = tpt._small()
    for q, shape in HAND + tpt.HAND + tpt.REFUSED[:2]:
        assert (trt.evaluate(q + "\n", rels), trt.total_rows(q + "\n", rels)) == tpt.brute(q + "\n", rels), shape
    nulls = sum(trt.evaluate(q + "\n", rels).startswith("NULL") for q, _ in HAND)
    assert nulls == NULLS                                # the table is not passing on NULLs: 2 of 21 lines
    for q, shape in BANDS + [(CYCLE, "a cycle")]:
        assert trt.evaluate(q + "\n", rels) is None, shape


def test_truth_of_single_links_is_theta_truth():
    for fixture in trt.CORPUS:
        rels, cases, want, rows = tt.corpus(fixture)
        _, _, twant, trows = trt.corpus(fixture)
        for c, w, r, tw, tr in zip(cases, want, rows, twant, trows):
            assert tw is not None, c["input"]            # no corpus case is a band or a cycle
            if w is not None:
                assert (tw, tr) == (w, r), c["input"]


@pytest.mark.parametrize("optional", ["all", "none"])
@pytest.mark.parametrize("fixture", list(trt.CORPUS))
def test_every_inequality_case_is_answered(fixture, optional):
    rels, cases, want, rows = trt.corpus(fixture)
    _, _, theta_want, _ = tt.corpus(fixture)
    eng = _engine(rels, optional)
    for c, w, r, tw in zip(cases, want, rows, theta_want):
        assert eng.run_theta_tree(c["input"]) == (w, 0, r), c["input"]
        if tw is None:                                   # the shape theta mode refuses: a number now
            assert r == FORMERLY_REFUSED[fixture] and "NULL" not in w, c["input"]
            assert eng.run_theta(c["input"])[:2] == ("", QE_ENOTSUP)
    assert sum(tw is None for tw in theta_want) == (fixture in FORMERLY_REFUSED)
    assert eng.live_handles() == 0                       # the plan releases every array it made
    assert eng.allgather_calls == 0 and eng.theta_weights_calls == 0
    assert eng.wsums_calls > 0 and eng.weighted64_calls > 0 and eng.select_cmp_calls > 0
    assert (fixture in FORMERLY_REFUSED) == (eng.wsums_weighted_calls > 0)


@pytest.mark.parametrize("world", [2, 3])
def test_every_inequality_case_on_ranks(world):
    """N gloo ranks print one rank's bytes: each rank weighs its rows against the gathered far side"""
    answered = gathers = 0
    for fixture in trt.CORPUS:
        rels, cases, want, rows = trt.corpus(fixture)
        res, live, ag, _ = _run_world(rels, [c["input"] for c in cases], world)
        assert live == 0
        gathers += ag
        for c, w, r, got in zip(cases, want, rows, res):
            assert got == (w, 0, r), c["input"]
            answered += 1
    assert answered == 68 and gathers > 0


@pytest.mark.parametrize("optional", ["all", "none"])
def test_hand_written_shapes(optional):
    rels = tpt._small()
    eng = _engine(rels, optional)
    for q, shape in HAND + tpt.HAND + tpt.REFUSED[:2]:
        want, total = tpt.brute(q + "\n", rels)
        assert eng.run_theta_tree(q + "\n") == (want, 0, total), shape
    assert eng.live_handles() == 0


@pytest.mark.parametrize("world", [2, 3])
def test_hand_written_shapes_on_ranks(world):
    rels = tpt._small()
    table = HAND + tpt.REFUSED[:2]
    res, live, _, _ = _run_world(rels, [q + "\n" for q, _ in table], world)
    assert live == 0
    for (q, shape), got in zip(table, res):
        want, total = tpt.brute(q + "\n", rels)
        assert got == (want, 0, total), shape


def test_messages_follow_the_roots():
    """one theta_wsums call per directed message toward a root; a component that needs two different
    products of its incoming messages takes one more call per factor it cannot reuse"""
    rels = tpt._small()
    eng = _engine(rels)
    chain, star = "0 1 2|0.0<1.0&1.1<2.1|", "1 0 2 2|0.0<1.0&0.1>2.1&0.2<3.2|"
    for q, calls, weighted in ((chain + "0.1\n", 2, 1), (chain + "2.1\n", 2, 1), (chain + "0.1 2.1\n", 4, 2),
                               (chain + "1.1\n", 2, 0), (chain + "0.1 1.1 2.1\n", 5, 2),
                               (star + "0.0\n", 3, 0), (star + "1.1\n", 3, 1), (star + "1.1 0.2\n", 4, 1),
                               (star + "1.0 2.0 3.0\n", 8, 3), ("0 1|0.0<1.0|1.1\n", 1, 0),
                               ("0 1|0.0<1.0|0.1 1.1\n", 2, 0)):
        before, wbefore = eng.wsums_calls, eng.wsums_weighted_calls
        want, total = tpt.brute(q, rels)
        assert eng.run_theta_tree(q) == (want, 0, total), q
        assert (eng.wsums_calls - before, eng.wsums_weighted_calls - wbefore) == (calls, weighted), q
    assert eng.live_handles() == 0


def test_messages_gather_keys_and_weights_on_ranks():
    """a chain selected at one end on 2 ranks: C's keys for C -> B, then B's keys and U_B for B -> A"""
    rels = tpt._small()
    q = "0 1 2|0.0<1.0&1.1<2.1|0.1\n"
    res, live, gathers, calls = _run_world(rels, [q], 2)
    want, total = tpt.brute(q, rels)
    assert res == [(want, 0, total)] and live == 0
    assert (calls, gathers) == (2, 3)


def test_bands_and_cycles_are_refused():
    small = tpt._small()
    good = HAND[0][0] + "\n"
    want = trt.evaluate(good, small)
    for q, word in [(b, "band") for b, _ in BANDS] + [(CYCLE, "cycle")]:
        eng = _engine(small)
        assert eng.run_theta_tree(q + "\n") == ("", QE_ENOTSUP, 0), q
        assert word in eng.why(), q
        assert eng.run_theta_tree(good + q + "\n" + good)[:2] == (want, QE_ENOTSUP), q
        assert eng.live_handles() == 0
        assert eng.wsums_calls == 5                      # (decided on the text: only the first `good` ran)


def test_a_refused_shape_leaves_every_rank_together():
    small = tpt._small()
    good = HAND[0][0] + "\n"
    res, live, _, _ = _run_world(small, [good + BANDS[0][0] + "\n" + good, good + CYCLE + "\n", good], 2)
    assert live == 0
    want = trt.evaluate(good, small)
    assert [r[:2] for r in res] == [(want, QE_ENOTSUP), (want, QE_ENOTSUP), (want, 0)]


def test_sizes_past_the_exactness_bound_are_too_big():
    """an engine that reports inflated list lengths: nothing large is allocated"""
    rels = tpt._small()
    q = "0 1 2|0.0<1.0&1.1<2.1&0.2<9&1.2<9&2.2<9|0.1\n"  # (every binding filtered: its size is a list's length)
    eng = _engine(rels, inflate_lengths=1 << 26)         # 40, 23, 9 x 2^26: each below 2^32, the product 2^91
    assert eng.run_theta_tree(q) == ("", QE_ETOOBIG, 0)
    assert "2^64" in eng.why() and eng.wsums_calls == 0 and eng.live_handles() == 0
    eng = _engine(rels, inflate_lengths=1 << 27)         # 40 x 2^27 rows: a link side past 2^32
    assert eng.run_theta_tree(q) == ("", QE_ETOOBIG, 0)
    assert "2^32" in eng.why() and eng.wsums_calls == 0 and eng.live_handles() == 0
    eng = _engine(rels, inflate_lengths=1 << 26)         # a single link is bounded by its sides alone
    two = "0 1|0.0<1.0&0.2<9&1.2<9|0.1\n"
    assert eng.run_theta_tree(two)[1] == 0 and eng.live_handles() == 0


def test_an_engine_without_a_callback_is_invalid():
    rels = tpt._small()
    for kw in ({"tree_callbacks": False}, {"theta_callbacks": False}):
        eng = _engine(rels, **kw)
        assert eng.run_theta_tree("0 1 2|0.0<1.0&1.1<2.1|0.1\n")[:2] == ("", QE_EINVAL)
        assert eng.run_theta_tree("0 1|0.0=1.0|0.1\n")[:2] == ("", QE_EINVAL)
    eng = _engine(rels, tree_callbacks=False)            # theta mode reads neither of the two
    q = "0 1|0.0<1.0|0.1 1.1\n"
    assert eng.run_theta(q)[:2] == (tt.evaluate(q, rels), 0)


def test_theta_mode_still_refuses_the_chain():
    eng = _engine(tpt._small())
    for q, _ in tpt.REFUSED:
        assert eng.run_theta(q + "\n") == ("", QE_ENOTSUP, 0)
    assert eng.wsums_calls == 0


def test_single_links_print_theta_modes_bytes():
    for fixture in trt.CORPUS:
        rels, cases, want, _ = tt.corpus(fixture)
        eng = _engine(rels)
        for c, w in zip(cases, want):
            if w is not None:
                assert eng.run_theta_tree(c["input"]) == eng.run_theta(c["input"]), c["input"]
        assert eng.live_handles() == 0


def test_queries_without_an_inequality_print_the_relational_lines():
    """every fourth corpus case: theta-tree mode == relational mode, byte for byte, rows included"""
    for fixture in rt.CORPUS:
        rels, cases, want = rt.corpus(fixture)
        eng = _engine(rels)
        for c, w in list(zip(cases, want))[::4]:
            got = eng.run_theta_tree(c["input"])
            assert got[:2] == (w, 0), c["input"]
            assert got == eng.run_relational(c["input"]), c["input"]
        assert eng.wsums_calls == 0 and eng.weighted64_calls == 0 and eng.select_cmp_calls == 0
        assert eng.live_handles() == 0


def test_a_tree_is_never_materialised():
    """no materialisation limit applies to links"""
    rels = tpt._small()
    eng = _engine(rels)
    eng.set_global_limit(10)
    q = "0 1 2|0.0<1.0&1.1<2.1|0.1 2.1\n"
    want, total = tpt.brute(q, rels)
    assert total > 10 and eng.run_theta_tree(q) == (want, 0, total)
    assert eng.live_handles() == 0
