"""The plan's theta mode (include/qe_plan.h: qe_plan_run_text_theta) on CPU: the compiled plan of
libqeplan.so over the numpy engine of tests/plan_engine_theta.py, against theta truth
(tests/theta_truth.py, itself checked here against a brute-force nested-loop evaluator) -- for the
68 corpus cases with a column < / > column predicate, which the relational mode refuses."""
import queue

import numpy as np
import pytest
import torch.multiprocessing as mp

import goldens
import plan_engine as pe
import plan_engine_theta as pet
import rel_truth as rt
import theta_truth as tt

QE_EINVAL, QE_ETOOBIG, QE_ENOTSUP = -1, -5, -6
M64 = (1 << 64) - 1

# hand-written shapes on the small relations below: (query, rule of the semantics it exercises)
HAND = [
    ("0|0.0<0.1|0.2", "1: one binding, <"),
    ("0|0.0>0.1|0.2 0.0", "1: one binding, >"),
    ("0|0.1<0.1|0.0", "1: b.x < b.x keeps nothing"),
    ("1|0.2>0.2|0.0", "1: b.x > b.x keeps nothing"),
    ("0 1|0.0>0.1&0.0=1.0|0.2 1.2", "1: a filter before the binding joins"),
    ("0 1|1.1<1.2|0.2 1.0", "1: a filter, then a cross product"),
    ("0 1|0.0=1.0&0.1<1.1|0.2 1.2", "2: selection inside a component, <"),
    ("0 1|0.1>1.1&0.0=1.0|0.2 1.2", "2: written before the join that connects them, >"),
    ("0 1 2|0.0=1.0&1.1=2.1&0.2<2.2|0.1 2.0", "2: the ends of a chain of equi-joins"),
    ("0 1 2|0.2>2.2&0.0=1.0&1.1=2.1|1.2", "2: the same, written first"),
    ("0 1 2|0.0=1.0&0.1<1.1&1.2=2.2&0.0>2.0|0.1 1.1 2.1", "2: two selections, both operators"),
    ("0 1|0.0=1.0&0.1<1.1&0.1>1.1|0.2", "2: contradictory selections"),
    ("0 1|0.0<1.0|0.1 1.1", "3: a link of two whole relations, <"),
    ("0 1|0.0>1.0|0.1 1.2", "3: a link, >"),
    ("0 0|0.1<1.1|0.2 1.2", "3: a relation linked with itself"),
    ("0 1 2|0.0=1.0&1.1<2.1|0.2 1.2 2.2", "3: a joined component linked with a relation"),
    ("0 1 2|2.1>1.1&0.0=1.0|0.2 1.2 2.2", "3: the link written first"),
    ("0 1 2|0.0<1.0|0.1 1.1 2.1", "3: a third, unlinked component multiplies"),
    ("0 1 2 0|0.0<1.0&2.0>3.0|0.1 1.1 2.1 3.2", "3: two links between two pairs"),
    ("0 1 2 1|0.0=1.0&2.0=3.0&1.1<3.1|0.2 1.2 2.2 3.2", "3: a link of two joined components"),
    ("0 1|0.0<1.0&0.1>3&1.2<5|0.2 1.2", "3: filters on both sides of a link"),
    ("0 1|0.0<1.0&1.0<1|0.1", "3: no pair, NULL"),
    ("0 1|0.0>1.0&0.0<1|0.1 1.1", "3: no pair, NULL"),
    ("0 1 2|0.0=1.0&0.1>1.1&1.2<2.2|0.0 1.1 2.2", "2 + 3: a selection and a link"),
    ("0 1|0.2<0.1&0.0>1.0&1.1>1.2|0.2 1.0", "1 + 3: filters on one binding each and a link"),
]
REFUSED = [
    ("0 1 2|0.0<1.0&1.1<2.1|0.1", "a chain"),
    ("0 1 2|0.0<1.0&0.1>2.1|0.1", "a component with two links"),
    ("0 1|0.0<1.0&0.1>1.1|0.1", "a band"),
    ("0 1 2|0.0=1.0&0.1<2.1&1.1>2.2|0.1", "a band between two components"),
]


def _small():
    """3 relations of 3 columns, at most 40 rows, values in [0, 8): ties and matches abound"""
    rng = np.random.default_rng(7)
    return [[rng.integers(0, 8, n).astype(np.uint64) for _ in range(3)] for n in (40, 23, 9)]


def brute(line: str, relations):
    """(line, total): the cross product of every binding, nested-loop style, every predicate a mask"""
    rels, cmps, filters, sels = tt.parse(line)
    col = lambda b, c: relations[rels[b]][c]
    idx = np.indices([len(col(b, 0)) for b in range(len(rels))]).reshape(len(rels), -1)
    keep = np.ones(idx.shape[1], dtype=bool)
    for b, c, op, v in filters:
        keep &= tt._cmp(col(b, c)[idx[b]], op, np.uint64(v))
    for b1, c1, op, b2, c2 in cmps:
        keep &= tt._cmp(col(b1, c1)[idx[b1]], op, col(b2, c2)[idx[b2]])
    total = int(keep.sum())
    if total == 0:
        return "NULL " * len(sels) + "\n", 0
    return "".join(f"{int(np.sum(col(b, c)[idx[b][keep]], dtype=np.uint64)) & M64} " for b, c in sels) + "\n", total


def _run_world(rels, queries, world, opts=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = pe.free_port()
    procs = [ctx.Process(target=pet.worker, args=(r, world, port, rels, queries, q, opts)) for r in range(world)]
    for p in procs:
        p.start()
    res = None
    try:
        # a rank that dies (a library without the theta entry points, say) never reports: notice its
        # exit at once instead of waiting for a result that cannot come
        while res is None:
            try:
                res = q.get(timeout=0.2)
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a rank exited with {dead} before rank 0 reported"
                if all(p.exitcode == 0 for p in procs):
                    res = q.get(timeout=5)               # (reported just before the last exit)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(timeout=10)
    return res


def test_truth_is_the_nested_loops():
    rels = _small()
    for q, shape in HAND:
        assert (tt.evaluate(q + "\n", rels), tt.total_rows(q + "\n", rels)) == brute(q + "\n", rels), shape
    nulls = sum(tt.evaluate(q + "\n", rels).startswith("NULL") for q, _ in HAND)
    assert 4 <= nulls <= 6                               # the table is not passing on NULLs
    for q, shape in REFUSED:
        assert tt.evaluate(q + "\n", rels) is None, shape


def test_truth_without_an_inequality_is_the_relational_truth():
    for fixture in rt.CORPUS:
        rels, cases, want = rt.corpus(fixture)
        for c, w in list(zip(cases, want))[::4]:
            assert tt.evaluate(c["input"], rels) == w, c["input"]
            assert tt.total_rows(c["input"], rels) == rt.total_rows(c["input"], rels), c["input"]


def test_corpus_is_what_the_issue_counted():
    """68 cases: 55 numeric lines, 11 all-NULL lines (5 + 3 + 3), 2 refused shapes (fuzz_a, fuzz_c)"""
    numeric = nulls = refused = 0
    per_fixture = {}
    for fixture, count in tt.CORPUS.items():
        _, cases, want, _ = tt.corpus(fixture)
        assert len(cases) == count
        n = sum(w is not None and set(w.split()) == {"NULL"} for w in want)
        r = sum(w is None for w in want)
        per_fixture[fixture] = (n, r)
        nulls += n
        refused += r
        numeric += len(cases) - n - r
    assert (numeric, nulls, refused) == (55, 11, 2)
    assert per_fixture == {"fuzz_a": (5, 1), "fuzz_b": (3, 0), "fuzz_c": (3, 1)}


@pytest.mark.parametrize("optional", ["all", "none"])
@pytest.mark.parametrize("fixture", list(tt.CORPUS))
def test_every_inequality_case_is_the_theta_answer(fixture, optional):
    rels, cases, want, rows = tt.corpus(fixture)
    on = optional == "all"
    eng = pet.NumpyPlanEngineTheta(rels, 0, 1, fused_scan=on, join_carry=on, join_sums=on, values=on, join_agg=on,
                                   key_carry=on)
    numeric = refused = 0
    for c, w, r in zip(cases, want, rows):
        out, rc, got_rows = eng.run_theta(c["input"])
        if w is None:
            assert (out, rc) == ("", QE_ENOTSUP), c["input"]
            assert "link" in eng.why() or "band" in eng.why()
            refused += 1
            continue
        assert (out, rc) == (w, 0), c["input"]
        assert got_rows == r, c["input"]
        numeric += set(w.split()) != {"NULL"}
    assert eng.live_handles() == 0                       # the plan releases every array it made
    assert eng.allgather_calls == 0                      # never at one rank
    assert eng.theta_weights_calls > 0 and eng.weighted_calls > 0 and eng.select_cmp_calls > 0
    assert (numeric, refused) == {"fuzz_a": (23, 1), "fuzz_b": (14, 0), "fuzz_c": (18, 1)}[fixture]


@pytest.mark.parametrize("world", [2, 3])
def test_every_inequality_case_on_ranks(world):
    """N gloo ranks print one rank's bytes: each rank weighs its rows against the gathered other side"""
    numeric = refused = gathers = 0
    for fixture in tt.CORPUS:
        rels, cases, want, rows = tt.corpus(fixture)
        res, live, ag = _run_world(rels, [c["input"] for c in cases], world)
        assert live == 0
        gathers += ag
        for c, w, r, (out, rc, got_rows) in zip(cases, want, rows, res):
            if w is None:
                assert (out, rc) == ("", QE_ENOTSUP), c["input"]
                refused += 1
                continue
            assert (out, rc) == (w, 0), c["input"]
            assert got_rows == r, c["input"]
            numeric += set(w.split()) != {"NULL"}
    assert numeric >= 55 and refused == 2
    assert gathers > 0


@pytest.mark.parametrize("optional", ["all", "none"])
def test_hand_written_shapes(optional):
    rels = _small()
    on = optional == "all"
    eng = pet.NumpyPlanEngineTheta(rels, 0, 1, fused_scan=on, join_carry=on, join_sums=on, values=on, join_agg=on,
                                   key_carry=on)
    for q, shape in HAND:
        want, total = brute(q + "\n", rels)
        assert eng.run_theta(q + "\n") == (want, 0, total), shape
    assert eng.live_handles() == 0


def test_hand_written_shapes_on_three_ranks():
    rels = _small()
    res, live, _ = _run_world(rels, [q + "\n" for q, _ in HAND], 3)
    assert live == 0
    for (q, shape), got in zip(HAND, res):
        want, total = brute(q + "\n", rels)
        assert got == (want, 0, total), shape


def test_refused_shapes_end_the_batch_with_the_lines_before_them():
    refused = [(c["input"], rels) for f in tt.CORPUS for rels, cases, want, _ in [tt.corpus(f)]
               for c, w in zip(cases, want) if w is None]
    assert len(refused) == 2
    small = _small()
    good = HAND[12][0] + "\n"
    for q, rels in refused + [(q + "\n", small) for q, _ in REFUSED]:
        eng = pet.NumpyPlanEngineTheta(rels, 0, 1)
        want = tt.evaluate(good, rels)
        assert eng.run_theta(good + q + good)[:2] == (want, QE_ENOTSUP), q
        assert eng.why()                                 # qe_plan_why names the reason
        assert eng.live_handles() == 0
    eng = pet.NumpyPlanEngineTheta(small, 0, 1)
    eng.run_theta(REFUSED[0][0] + "\n")
    assert "two or more" in eng.why()
    eng.run_theta(REFUSED[2][0] + "\n")
    assert "band" in eng.why()


def test_refused_shapes_leave_every_rank_together():
    small = _small()
    good = HAND[12][0] + "\n"
    res, live, _ = _run_world(small, [good + REFUSED[0][0] + "\n" + good, good], 2)
    assert live == 0
    assert res[0][:2] == (tt.evaluate(good, small), QE_ENOTSUP)
    assert res[1][:2] == (tt.evaluate(good, small), 0)


def test_an_engine_without_the_callbacks_is_invalid():
    rels = _small()
    eng = pet.NumpyPlanEngineTheta(rels, 0, 1, theta_callbacks=False)
    assert eng.run_theta("0 1|0.0<1.0|0.1\n")[:2] == ("", QE_EINVAL)
    assert eng.run_theta("0 1|0.0=1.0|0.1\n")[:2] == ("", QE_EINVAL)
    # the relational entry point reads none of them
    assert eng.run_relational("0 1|0.0=1.0|0.1\n")[:2] == (rt.evaluate("0 1|0.0=1.0|0.1\n", rels), 0)


def test_the_relational_entry_point_still_refuses():
    eng = pet.NumpyPlanEngineTheta(_small(), 0, 1)
    assert eng.run_relational("0 1|0.0<1.0|0.1\n") == ("", QE_ENOTSUP, 0)


def test_queries_without_an_inequality_print_the_relational_lines():
    """every fourth corpus case: theta mode == relational mode, byte for byte, rows included"""
    for fixture in rt.CORPUS:
        rels, cases, want = rt.corpus(fixture)
        eng = pet.NumpyPlanEngineTheta(rels, 0, 1)
        for c, w in list(zip(cases, want))[::4]:
            got = eng.run_theta(c["input"])
            assert got[:2] == (w, 0), c["input"]
            assert got == eng.run_relational(c["input"]), c["input"]
        assert eng.theta_weights_calls == 0 and eng.select_cmp_calls == 0 and eng.weighted_calls == 0
        assert eng.live_handles() == 0


def test_a_link_is_never_materialised():
    """no materialisation limit applies to a link; its equi-joins keep theirs"""
    rels = _small()
    eng = pet.NumpyPlanEngineTheta(rels, 0, 1)
    eng.set_global_limit(10)
    q = "0 1|0.0<1.0|0.1 1.1\n"
    want, total = brute(q, rels)
    assert total > 10 and eng.run_theta(q) == (want, 0, total)
    assert eng.run_theta("0 1 2|0.0=1.0&1.1<2.1|0.2 1.2 2.2\n")[:2] == ("", QE_ETOOBIG)
    assert eng.live_handles() == 0


def test_the_second_side_is_weighed_only_when_a_select_reads_it():
    rels = _small()
    eng = pet.NumpyPlanEngineTheta(rels, 0, 1)
    for q, calls in (("0 1|0.0<1.0|0.1\n", 1), ("0 1|0.0<1.0|1.1\n", 2), ("0 1|0.0<1.0|0.1 1.1\n", 2)):
        before = eng.theta_weights_calls
        want, total = brute(q, rels)
        assert eng.run_theta(q) == (want, 0, total), q
        assert eng.theta_weights_calls - before == calls, q
    assert eng.live_handles() == 0
