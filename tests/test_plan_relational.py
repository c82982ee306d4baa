"""The plan's relational mode (include/qe_plan.h: qe_plan_run_text_relational) on CPU: the compiled
plan of libqeplan.so over the numpy engine of tests/plan_engine_rel.py, against relational truth
(tests/rel_truth.py, itself checked here against oracle/truth.py) -- for every single-query case of
the fuzz and known-answer fixtures, the reference's wrong (W) and exiting (X) ones included."""
import numpy as np
import pytest
import torch.multiprocessing as mp

import goldens
import plan_engine as pe
import plan_engine_rel as per
import rel_truth as rt

QE_EINVAL, QE_ETOOBIG, QE_ENOTSUP = -1, -5, -6

HAND = rt.HAND


def _fuzz_b():
    return goldens.dataset(goldens.load(f"{goldens.GOLDEN_DIR}/fuzz_b.json")["dataset"])[0]


def _run_world(rels, queries, world, opts=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = pe.free_port()
    procs = [ctx.Process(target=per.worker, args=(r, world, port, rels, queries, q, opts)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("fixture", list(rt.CORPUS))
def test_numpy_truth_is_the_oracles(fixture):
    pytest.importorskip("pandas")
    from oracle import truth
    rels, cases, want = rt.corpus(fixture)
    assert len(cases) == rt.CORPUS[fixture]
    for c, w in zip(cases, want):
        assert truth.evaluate(c["input"], rels) == w, c["input"]


def test_corpus_is_what_the_issue_counted():
    """503 cases run; 79 of them are the reference's wrong or exiting ones (they fail on any
    executor that reproduces the reference), 72 hold a predicate inside a component"""
    n = w = inside = 0
    for fixture, count in rt.CORPUS.items():
        cases = rt.corpus_cases(fixture)
        assert len(cases) == count
        n += len(cases)
        w += sum(c.get("class") in ("W", "X") for c in cases)
        inside += sum(rt.in_component(c["input"]) for c in cases)
    assert (n, w, inside) == (503, 79, 72)


@pytest.mark.parametrize("optional", ["all", "none"])
@pytest.mark.parametrize("fixture", list(rt.CORPUS))
def test_every_case_is_the_relational_answer(fixture, optional):
    """with the engine's optional entries (fused scans, carried bindings, aggregate last joins,
    values and keys riding with the rows) and without them"""
    rels, cases, want = rt.corpus(fixture)
    assert len(cases) == rt.CORPUS[fixture]
    on = optional == "all"
    eng = per.NumpyPlanEngineRel(rels, 0, 1, fused_scan=on, join_carry=on, join_sums=on, values=on, join_agg=on,
                                 key_carry=on)
    for c, w in zip(cases, want):
        out, rc, rows = eng.run_relational(c["input"])
        assert (out, rc) == (w, 0), c["input"]
        assert rows == rt.total_rows(c["input"], rels), c["input"]
    assert eng.live_handles() == 0                     # the plan releases every array it made
    assert eng.select_eq_calls > 0
    if fixture != "known_answers":
        assert eng.select_eq_lists >= 3                # a component of three bindings compacted at once
        assert (eng.sums_calls > 0) == on              # the aggregate last joins stay in use
        assert (eng.agg_calls > 0) == on


@pytest.mark.parametrize("world", [2, 3])
def test_every_fifth_case_on_ranks(world):
    """N gloo ranks print one rank's bytes (the selections are rank-local, sizes all-reduced)"""
    for fixture in rt.CORPUS:
        rels, cases, want = rt.corpus(fixture)
        pick = list(range(0, len(cases), 5))
        one = per.NumpyPlanEngineRel(rels, 0, 1)
        res, live = _run_world(rels, [cases[i]["input"] for i in pick], world)
        assert live == 0
        for i, (out, rc, rows) in zip(pick, res):
            assert (out, rc) == (want[i], 0), cases[i]["input"]
            assert (out, rc, rows) == one.run_relational(cases[i]["input"]), cases[i]["input"]


@pytest.mark.parametrize("optional", ["all", "none"])
def test_hand_written_shapes(optional):
    rels = _fuzz_b()
    on = optional == "all"
    eng = per.NumpyPlanEngineRel(rels, 0, 1, fused_scan=on, join_carry=on, join_sums=on, values=on, join_agg=on,
                                 key_carry=on)
    for q, want, shape in HAND:
        assert rt.evaluate(q + "\n", rels) == want + "\n", shape
        assert eng.run_relational(q + "\n")[:2] == (want + "\n", 0), shape
    assert eng.live_handles() == 0
    # a batch: one line per query, no filter count lines, F lines skipped
    text = "".join(q + "\n" for q, _, _ in HAND[:4]) + "F\n" + HAND[4][0] + "\n"
    assert eng.run_relational(text)[:2] == ("".join(w + "\n" for _, w, _ in HAND[:5]), 0)


def test_hand_written_shapes_on_two_ranks():
    rels = _fuzz_b()
    res, live = _run_world(rels, [q + "\n" for q, _, _ in HAND], 2)
    assert live == 0
    for (q, want, shape), (out, rc, _) in zip(HAND, res):
        assert (out, rc) == (want + "\n", 0), shape


def test_rows_is_the_product_of_the_component_sizes():
    rels = _fuzz_b()
    eng = per.NumpyPlanEngineRel(rels, 0, 1)
    assert eng.run_relational("0 1 2 3 4|0.0=0.0|0.1\n")[2] == 3000 ** 5
    # saturated, and the printed product wraps mod 2^64
    many = " ".join(["0"] * 6)
    out, rc, rows = eng.run_relational(many + "|0.0=0.0|0.1\n")
    assert (rc, rows) == (0, (1 << 64) - 1)
    s = int(np.sum(rels[0][1], dtype=np.uint64))
    assert out == f"{(s * 3000 ** 5) & ((1 << 64) - 1)} \n"
    assert eng.run_relational("0 1|0.0>4000000000&0.0=1.0|0.1\n")[2] == 0


def test_errors_end_the_batch_with_the_output_before_them():
    rels = _fuzz_b()
    eng = per.NumpyPlanEngineRel(rels, 0, 1)
    good, want = HAND[0][0] + "\n", HAND[0][1] + "\n"
    assert eng.run_relational("0 1|0.0<1.0|0.1\n") == ("", QE_ENOTSUP, 0)
    assert eng.run_relational("0 1|0.0=1.0&0.1>1.1|0.1\n")[:2] == ("", QE_ENOTSUP)
    assert eng.run_relational(good + "0 1|0.0<1.0|0.1\n" + good)[:2] == (want, QE_ENOTSUP)
    for bad in ("0 1|0.0=1.7|0.1\n", "0 9|0.0=1.0|0.1\n", "0 1|0.0=2.0|0.1\n", "0 1|0.0=1.0|2.1\n",
                "0 1|0.0=1.0|1.3\n", "0 1|0.5>7|0.1\n"):
        assert eng.run_relational(good + bad + good)[:2] == (want, QE_EINVAL), bad
    assert eng.live_handles() == 0


def test_a_join_beyond_the_limit_has_no_fallback():
    """both sides of a 3-way join selected, so no aggregate form covers its joins"""
    rels = _fuzz_b()
    q = "0 1 2|0.1=1.1&1.1=2.1|0.2 1.2 2.2\n"
    eng = per.NumpyPlanEngineRel(rels, 0, 1)
    assert eng.run_relational(q)[:2] == (rt.evaluate(q, rels), 0)
    eng.set_global_limit(1000)
    assert eng.run_relational(q)[:2] == ("", QE_ETOOBIG)
    assert eng.live_handles() == 0
    # an aggregate last join materialises nothing: no limit applies to it
    q2 = "0 1|0.1=1.1|0.2 1.2\n"
    assert eng.run_relational(q2)[:2] == (rt.evaluate(q2, rels), 0)


def test_the_existing_entry_points_take_the_shorter_struct():
    """qe_plan_run_text never reads select_eq: the engine of tests/plan_engine.py (no such field)
    and this one print the same bytes"""
    rels = _fuzz_b()
    q = "0 1|0.0=1.0&0.2>2000000000|0.1 1.1\n"
    assert pe.NumpyPlanEngine(rels, 0, 1).run(q)[:2] == per.NumpyPlanEngineRel(rels, 0, 1).run(q)[:2]
