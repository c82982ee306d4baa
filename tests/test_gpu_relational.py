"""The relational mode on the GPU: qe_select_equal against numpy, and qe_run_queries_relational --
one rank, in-process ranks, the lanes and the `queries` binary -- against relational truth
(tests/rel_truth.py) on every single-query case of the fuzz and known-answer fixtures, the ones the
reference gets wrong (class W) or exits on (class X) included."""
import json
import os
import subprocess

import numpy as np
import pytest

import goldens
import rel_truth as rt
from qe import datagen as dg
from qe import lib

pytestmark = pytest.mark.gpu

HAND = rt.HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = os.path.join(ROOT, "query-compiler-executor_amd", "build", "queries")
_loaded = {"key": None}


def _load(ctx, ds):
    key = json.dumps(ds, sort_keys=True)
    if _loaded["key"] != key:
        ctx.drop_relations()
        rels, _ = goldens.dataset(ds)
        for cols in rels:
            ctx.load_relation(cols)
        _loaded["key"] = key


def _load_fixture(ctx, fixture):
    _load(ctx, goldens.load(f"{goldens.GOLDEN_DIR}/{fixture}.json")["dataset"])


# ---- qe_select_equal ----------------------------------------------------------------------------

def _select_case(ctx, keep, wide, seed):
    """a relation of two columns and two rowid lists a, b (permutations of its rows) such that
    colA[a[i]] == colB[b[i]] exactly where keep[i]; wide: values of 2^32 and more, a dropped
    position differing from its partner in the high word only"""
    n = len(keep)
    rng = np.random.default_rng(seed)
    rows = n + 7
    a = rng.permutation(rows)[:n].astype(np.uint32)
    b = rng.permutation(rows)[:n].astype(np.uint32)
    colA = rng.integers(0, 1 << 31, rows, dtype=np.uint64)
    if wide:
        colA |= rng.integers(1, 1 << 20, rows, dtype=np.uint64) << np.uint64(32)
    colB = rng.integers(0, 1 << 31, rows, dtype=np.uint64) | np.uint64(1 << 31)      # no chance match
    flip = np.uint64(1 << 32) if wide else np.uint64(1)
    colB[b] = np.where(keep, colA[a], colA[a] ^ flip)
    ctx.drop_relations()
    _loaded["key"] = None
    rel = ctx.load_relation([colA, colB])
    return colA, colB, a, b, ctx.column(rel, 0), ctx.column(rel, 1)


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating"])
def test_select_equal_against_numpy(ctx, pattern, wide):
    T = ctx.select_equal_tile()
    nmax = 3 * T + 5
    keep = {"none": np.zeros(nmax, bool), "all": np.ones(nmax, bool), "alternating": np.arange(nmax) % 2 == 0}[pattern]
    colA, colB, a, b, dA, dB = _select_case(ctx, keep, wide, 7)
    c = np.random.default_rng(8).integers(0, 1 << 32, nmax, dtype=np.uint64).astype(np.uint32)
    for n in (0, 1, 3, T - 1, T, T + 1, 3 * T + 5):
        want = colA[a[:n]] == colB[b[:n]]
        assert np.array_equal(want, keep[:n])
        la, lb, lc = (ctx.list_from_host(x[:n]) for x in (a, b, c))
        # one list that is neither a nor b; a and b themselves; one more than a launch carries
        for lists, host in (([lc], [c]), ([la, lb], [a, b]), ([la, lb, lc], [a, b, c])):
            outs = ctx.select_equal(dA, la, dB, lb, lists)
            for o, h in zip(outs, host):
                assert np.array_equal(ctx.list_to_host(o), h[:n][want]), (n, len(lists))   # order kept
                ctx.list_free(o)
        for l in (la, lb, lc):
            ctx.list_free(l)


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
def test_select_equal_aliased_and_positional_lists(ctx, wide):
    T = ctx.select_equal_tile()
    n = T + 1
    keep = np.arange(n) % 3 == 0
    colA, colB, a, b, dA, dB = _select_case(ctx, keep, wide, 9)
    la, lb = ctx.list_from_host(a), ctx.list_from_host(b)
    # a is b: one binding's two columns compared row by row
    colB2 = colB.copy()
    colB2[a] = np.where(keep, colA[a], colB2[a])
    rel = ctx.load_relation([colB2])
    want = colA[a] == colB2[a]
    assert want.sum() == keep.sum()
    (o,) = ctx.select_equal(dA, la, ctx.column(rel, 0), la, [la])
    assert np.array_equal(ctx.list_to_host(o), a[want])
    ctx.list_free(o)
    # a NULL: position i is colA's row i
    want = colA[:n] == colB[b]
    o1, o2 = ctx.select_equal(dA, None, dB, lb, [lb, la])
    assert np.array_equal(ctx.list_to_host(o1), b[want]) and np.array_equal(ctx.list_to_host(o2), a[want])
    for l in (o1, o2, la, lb):
        ctx.list_free(l)
    # lists of different lengths are refused
    short = ctx.list_from_host(a[:5])
    lb = ctx.list_from_host(b)
    with pytest.raises(lib.QEError):
        ctx.select_equal(dA, short, dB, lb, [lb])
    ctx.list_free(short)
    ctx.list_free(lb)


# ---- the executor -------------------------------------------------------------------------------

def _batch(fixture):
    rels, cases, want = rt.corpus(fixture)
    assert len(cases) == rt.CORPUS[fixture]            # nothing skipped silently
    return rels, "".join(c["input"] for c in cases), "".join(want), cases, want


def _explain(run, cases, want):
    """the first case that differs, run on its own (a batch's bytes do not say which line is wrong)"""
    for c, w in zip(cases, want):
        got = run(c["input"])
        assert got == (w, 0), c["input"]


@pytest.mark.parametrize("fixture", list(rt.CORPUS))
def test_relational_batch_is_truth(ctx, fixture):
    rels, text, want, cases, lines = _batch(fixture)
    _load_fixture(ctx, fixture)
    run = lambda t: ctx.run_relational(t)
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)
    assert ctx.last_result_rows() == rt.total_rows(cases[-1]["input"], rels)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("fixture", list(rt.CORPUS))
def test_relational_batch_on_local_ranks_is_truth(ctx, fixture, nranks):
    rels, text, want, cases, lines = _batch(fixture)
    _load_fixture(ctx, fixture)
    run = lambda t: ctx.run_relational_local(t, nranks)[:2]
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)


def _binary(paths, queries, env):
    r = subprocess.run([QUERIES], input=dg.protocol_input(paths, queries).encode(), capture_output=True, timeout=600,
                       env=dict(os.environ, QE_RELATIONAL="1", **env))
    return r.stdout.decode("latin-1"), r.returncode


@pytest.mark.parametrize("env", [{}, {"QE_WORKERS": "1"}, {"QE_LOCAL_RANKS": "2"}, {"QE_GPUS": "1"}],
                         ids=["lanes", "one-lane", "local2", "ranks1"])
def test_binary_relational_mode(env):
    doc = goldens.load(f"{goldens.GOLDEN_DIR}/known_answers.json")
    _, paths = goldens.dataset(doc["dataset"])
    _, text, want, _, _ = _batch("known_answers")
    assert _binary(paths, text, env) == (want, 0)


def test_binary_relational_mode_ends_the_batch_at_a_refused_query():
    doc = goldens.load(f"{goldens.GOLDEN_DIR}/known_answers.json")
    _, paths = goldens.dataset(doc["dataset"])
    _, _, _, cases, lines = _batch("known_answers")
    text = cases[0]["input"] + "0 1|0.0<1.0|0.1\n" + cases[1]["input"]
    assert _binary(paths, text, {"QE_WORKERS": "1"}) == (lines[0], 70)


def test_c4_on_lanes_is_truth(ctx):
    """every case of c4 the reference gets wrong (169) and every fourth it gets right, on 4 lanes"""
    doc = goldens.load(f"{goldens.GOLDEN_DIR}/c4.json")
    rels, _ = goldens.dataset(doc["dataset"])
    wrong = [c for c in doc["cases"] if c.get("class") == "W"]
    right = [c for c in doc["cases"] if c.get("class") == "T"][::4]
    assert len(wrong) == 169 and len(right) == 177
    cases = wrong + right
    lines = [rt.evaluate(c["input"], rels) for c in cases]
    assert sum(c["stdout"] != w for c, w in zip(wrong, lines)) == 169      # truly not the reference's bytes
    _load(ctx, doc["dataset"])
    run = lambda t: ctx.run_lanes(t, 4, executor=lib.QE_EXEC_RELATIONAL)
    text, want = "".join(c["input"] for c in cases), "".join(lines)
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)


def test_hand_written_shapes(ctx):
    _load_fixture(ctx, "fuzz_b")
    for q, want, shape in HAND:
        assert ctx.run_relational(q + "\n") == (want + "\n", 0), shape
        assert ctx.run_relational_local(q + "\n", 2)[:2] == (want + "\n", 0), shape
    text, want = "".join(q + "\n" for q, _, _ in HAND), "".join(w + "\n" for _, w, _ in HAND)
    assert ctx.run_relational(text) == (want, 0)
    assert ctx.run_lanes(text, 4, executor=lib.QE_EXEC_RELATIONAL) == (want, 0)
    assert ctx.run_lanes(text, 1, executor=lib.QE_EXEC_RELATIONAL) == (want, 0)


def test_errors(ctx):
    _load_fixture(ctx, "fuzz_b")
    good, want = HAND[0][0] + "\n", HAND[0][1] + "\n"
    assert ctx.run_relational("0 1|0.0<1.0|0.1\n") == ("", lib.QE_ENOTSUP)
    assert ctx.run_relational("0 1|0.0=1.0|0.7\n") == ("", lib.QE_EINVAL)           # an out-of-range column
    for run in (lambda t: ctx.run_relational(t), lambda t: ctx.run_relational_local(t, 2)[:2],
                lambda t: ctx.run_lanes(t, 4, executor=lib.QE_EXEC_RELATIONAL)):
        assert run(good + "0 1|0.0<1.0|0.1\n" + good) == (want, lib.QE_ENOTSUP)
        assert run(good + good + "0 1|0.0=1.3|0.1\n" + good) == (want + want, lib.QE_EINVAL)


def test_join_beyond_the_materialisation_limit(ctx):
    """both sides of a 3-way join selected: QE_ETOOBIG (there is no fallback executor), or an
    aggregate form with the right sums"""
    _load_fixture(ctx, "fuzz_b")
    rels, _, _ = rt.corpus("fuzz_b")
    q = "0 1 2|0.1=1.1&1.1=2.1|0.2 1.2 2.2\n"
    assert ctx.run_relational(q) == (rt.evaluate(q, rels), 0)
    ctx.set_materialize_limit(1000)
    try:
        out, rc = ctx.run_relational(q)
        assert (out, rc) in (("", lib.QE_ETOOBIG), (rt.evaluate(q, rels), 0))
        out, rc, _ = ctx.run_relational_local(q, 2)
        assert (out, rc) in (("", lib.QE_ETOOBIG), (rt.evaluate(q, rels), 0))
    finally:
        ctx.set_materialize_limit(0x7FFFFFFF)
    assert ctx.run_relational(q) == (rt.evaluate(q, rels), 0)
