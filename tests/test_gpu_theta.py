"""The theta mode on the GPU: qe_theta_counts, qe_select_compare and qe_allgather_u64 against numpy,
and qe_run_queries_theta -- one rank, in-process ranks, the lanes and the `queries` binary -- against
theta truth (tests/theta_truth.py) on the 68 corpus cases with a column < / > column predicate."""
import json
import os
import subprocess

import numpy as np
import pytest

import goldens
import rel_truth as rt
import theta_truth as tt
from qe import datagen as dg
from qe import lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = os.path.join(ROOT, "query-compiler-executor_amd", "build", "queries")
MJ_TILE = 4096                                          # the merge tile qe_theta_counts walks R in
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


# ---- qe_theta_counts ----------------------------------------------------------------------------

def _keys(pattern, nR, nS, rng):
    if pattern == "equal":                              # every key equal on both sides: every count 0
        return np.full(nR, 77, np.uint64), np.full(nS, 77, np.uint64)
    if pattern == "single":                             # S one key, R straddling it
        return rng.integers(999, 1002, nR).astype(np.uint64), np.full(nS, 1000, np.uint64)
    if pattern == "dups":                               # heavy duplicates: a window wider than LDS
        return rng.integers(0, 64, nR).astype(np.uint64), rng.integers(0, 64, nS).astype(np.uint64)
    hi = lambda n: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    r, s = hi(nR) | np.uint64(1 << 32), hi(nS) | np.uint64(1 << 32)     # keys of 2^32 and more ...
    for a in (r, s):                                    # ... with 0 and 2^64 - 1 among them
        if len(a) > 2:
            a[0], a[1] = 0, np.uint64((1 << 64) - 1)
    if len(s) > 3:
        r[-1] = s[3]                                    # a tie between the sides
    return r, s


def _sorted_pairs(ctx, keys, rng):
    order = np.argsort(keys, kind="stable")
    val = rng.permutation(len(keys)).astype(np.uint32)
    p = ctx.pairs_from_host(keys[order], val)
    p.flags |= lib.PAIRS_SORTED
    return p, keys[order]


@pytest.mark.parametrize("pattern", ["equal", "single", "dups", "wide"])
def test_theta_counts_against_numpy(ctx, pattern):
    rng = np.random.default_rng(11)
    for nS in (0, 1, 8195, 50_000):
        for nR in (1, MJ_TILE - 1, MJ_TILE, MJ_TILE + 1, 3 * MJ_TILE + 5):
            rk, sk = _keys(pattern, nR, nS, rng)
            R, rs = _sorted_pairs(ctx, rk, rng)
            S, ss = _sorted_pairs(ctx, sk, rng)
            for op in "<>":
                want = tt.weights(rs, ss, op)
                pairs = ctx.theta_counts(R, S, op)
                got = ctx.counts_to_host(R.match, nR)
                assert np.array_equal(got, want), (pattern, nR, nS, op)
                assert pairs == int(want.sum()), (pattern, nR, nS, op)
                assert not R.flags & lib.PAIRS_MATCHED
                if pattern == "equal":
                    assert pairs == 0
            ctx.pairs_free(R)
            ctx.pairs_free(S)


def test_theta_counts_feeds_the_weighted_checksum_and_clears_matched(ctx):
    """the counts are what qe_checksum_weighted sums, and no equi-join's: QE_PAIRS_MATCHED is cleared"""
    rng = np.random.default_rng(12)
    n = MJ_TILE + 9
    col = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    ctx.drop_relations()
    _loaded["key"] = None
    rel = ctx.load_relation([col])
    rk, sk = rng.integers(0, 500, n).astype(np.uint64), rng.integers(0, 500, 3000).astype(np.uint64)
    order = np.argsort(rk, kind="stable")
    R = ctx.pairs_from_host(rk[order], order.astype(np.uint32))
    R.flags |= lib.PAIRS_SORTED
    S, _ = _sorted_pairs(ctx, sk, rng)
    assert ctx.merge_join_counts(R, S) >= 0 and R.flags & lib.PAIRS_MATCHED
    pairs = ctx.theta_counts(R, S, "<")
    assert not R.flags & lib.PAIRS_MATCHED
    w = tt.weights(rk, sk, "<")
    assert pairs == int(w.sum())
    with np.errstate(over="ignore"):
        assert ctx.checksum_weighted(ctx.column(rel, 0), R) == int(np.sum(col * w, dtype=np.uint64))
    # unsorted sides and other operators are refused
    U = ctx.pairs_from_host(rk, order.astype(np.uint32))
    for bad in (lambda: ctx.theta_counts(U, S, "<"), lambda: ctx.theta_counts(R, U, ">"),
                lambda: ctx.theta_counts(R, S, "=")):
        with pytest.raises(lib.QEError):
            bad()
    for p in (R, S, U):
        ctx.pairs_free(p)


# ---- qe_select_compare --------------------------------------------------------------------------

_NP = {"=": np.equal, "<": np.less, ">": np.greater}


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
def test_select_compare_against_numpy(ctx, wide):
    T = ctx.select_equal_tile()
    rng = np.random.default_rng(13)
    nmax = 2 * T + 7
    rows = nmax + 7
    colA = rng.integers(0, 16, rows).astype(np.uint64)
    colB = rng.integers(0, 16, rows).astype(np.uint64)
    if wide:                                            # the high words decide, the low words mislead
        colA = (colA << np.uint64(32)) | rng.integers(0, 1 << 32, rows, dtype=np.uint64)
        colB = (colB << np.uint64(32)) | rng.integers(0, 1 << 32, rows, dtype=np.uint64)
    ctx.drop_relations()
    _loaded["key"] = None
    rel = ctx.load_relation([colA, colB])
    dA, dB = ctx.column(rel, 0), ctx.column(rel, 1)
    a = rng.permutation(rows)[:nmax].astype(np.uint32)
    b = rng.permutation(rows)[:nmax].astype(np.uint32)
    if wide:                                            # some pairs equal in all 64 bits
        colB[b[::16]] = colA[a[::16]]
        ctx.drop_relations()
        rel = ctx.load_relation([colA, colB])
        dA, dB = ctx.column(rel, 0), ctx.column(rel, 1)
    a[5], b[9] = rows, rows + 100                       # a rowid past its column never matches
    extra = [rng.integers(0, 1 << 32, nmax, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    for n in (T - 1, T, T + 1, 2 * T + 7):
        ok = (a[:n] < rows) & (b[:n] < rows)
        va, vb = colA[np.minimum(a[:n], rows - 1)], colB[np.minimum(b[:n], rows - 1)]
        la, lb = ctx.list_from_host(a[:n]), ctx.list_from_host(b[:n])
        lx = [ctx.list_from_host(x[:n]) for x in extra]
        for op in "=<>":
            want = ok & _NP[op](va, vb)
            assert 0 < want.sum() < n
            for lists, host in (([lx[0]], [extra[0]]), ([la, lb], [a, b]), ([la, lb, lx[0]], [a, b, extra[0]]),
                                ([la, lb] + lx, [a, b] + extra)):                       # 1, 2, 3 and 5 lists
                outs = ctx.select_compare(dA, la, op, dB, lb, lists)
                for o, h in zip(outs, host):
                    assert np.array_equal(ctx.list_to_host(o), h[:n][want]), (n, op, len(lists))   # order kept
                    ctx.list_free(o)
            if op == "=":                               # '=' is qe_select_equal itself
                (o,) = ctx.select_equal(dA, la, dB, lb, [la])
                assert np.array_equal(ctx.list_to_host(o), a[:n][want])
                ctx.list_free(o)
        # a is b: one binding's two columns, row by row; x op x keeps nothing unless op is '='
        for op in "=<>":
            want = (a[:n] < rows) & _NP[op](va, colB[np.minimum(a[:n], rows - 1)])
            (o,) = ctx.select_compare(dA, la, op, dB, la, [la])
            assert np.array_equal(ctx.list_to_host(o), a[:n][want]), (n, op)
            ctx.list_free(o)
            (o,) = ctx.select_compare(dA, la, op, dA, la, [la])
            assert ctx.list_to_host(o).size == (int((a[:n] < rows).sum()) if op == "=" else 0)
            ctx.list_free(o)
        # a NULL: position i is colA's row i
        for op in "<>":
            want = (b[:n] < rows) & _NP[op](colA[:n], vb)
            o1, o2 = ctx.select_compare(dA, None, op, dB, lb, [lb, la])
            assert np.array_equal(ctx.list_to_host(o1), b[:n][want]) and np.array_equal(ctx.list_to_host(o2), a[:n][want])
            ctx.list_free(o1)
            ctx.list_free(o2)
        for l in [la, lb] + lx:
            ctx.list_free(l)
    la = ctx.list_from_host(a[:8])
    with pytest.raises(lib.QEError):                    # an operator that is none of the three
        ctx.select_compare(dA, la, "!", dB, la, [la])
    ctx.list_free(la)


def test_select_compare_reports_its_own_stage(ctx):
    rng = np.random.default_rng(14)
    col = rng.integers(0, 9, 5000).astype(np.uint64)
    ctx.drop_relations()
    _loaded["key"] = None
    rel = ctx.load_relation([col, col[::-1].copy()])
    l = ctx.list_from_host(np.arange(5000, dtype=np.uint32))
    ctx.set_profiling(True)
    ctx.reset_stats()
    try:
        for op in "=<>":
            (o,) = ctx.select_compare(ctx.column(rel, 0), l, op, ctx.column(rel, 1), l, [l])
            ctx.list_free(o)
        st = ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    assert st["select_equal"]["launches"] == 1 and st["select_compare"]["launches"] == 2
    ctx.list_free(l)


# ---- qe_allgather_u64 ---------------------------------------------------------------------------

@pytest.mark.parametrize("nranks", [2, 3])
def test_allgather_on_local_ranks(ctx, nranks):
    rng = np.random.default_rng(15)
    counts = [5000, 0, 37][:nranks]                     # unequal, one of them 0
    keys = [rng.integers(0, 1 << 63, n, dtype=np.uint64) for n in counts]
    g = lib.LocalComms(ctx.workers(nranks))
    try:
        res = g.allgather(keys)
        again = g.allgather(keys[::-1])                 # (the posted slots are reusable)
    finally:
        g.close()
    for r in res:
        assert np.array_equal(r, np.concatenate(keys))
    for r in again:
        assert np.array_equal(r, np.concatenate(keys[::-1]))


def test_allgather_without_a_communicator_is_a_copy(ctx):
    keys = np.arange(1000, dtype=np.uint64) * np.uint64(1 << 40)
    cm = lib.Comm.__new__(lib.Comm)
    cm.ctx, cm.lib, cm.h = ctx, ctx.lib, None
    assert np.array_equal(cm.allgather(keys), keys)
    assert cm.allgather(keys[:0]).size == 0


# ---- the executor -------------------------------------------------------------------------------

def _batch(fixture):
    """the fixture's inequality cases the mode answers, as one batch (a refused one would end it)"""
    rels, cases, want, rows = tt.corpus(fixture)
    assert len(cases) == tt.CORPUS[fixture]             # nothing skipped silently
    keep = [i for i, w in enumerate(want) if w is not None]
    cases, want, rows = [cases[i] for i in keep], [want[i] for i in keep], [rows[i] for i in keep]
    return rels, "".join(c["input"] for c in cases), "".join(want), cases, want, rows


def _refused(fixture):
    _, cases, want, _ = tt.corpus(fixture)
    return [c["input"] for c, w in zip(cases, want) if w is None]


def _explain(run, cases, want):
    """the first case that differs, run on its own (a batch's bytes do not say which line is wrong)"""
    for c, w in zip(cases, want):
        assert run(c["input"]) == (w, 0), c["input"]


def test_corpus_is_not_passing_on_nulls():
    numeric = refused = 0
    for fixture in tt.CORPUS:
        _, _, _, _, want, _ = _batch(fixture)
        numeric += sum(set(w.split()) != {"NULL"} for w in want)
        refused += len(_refused(fixture))
    assert numeric >= 55 and refused == 2


@pytest.mark.parametrize("fixture", list(tt.CORPUS))
def test_theta_batch_is_truth(ctx, fixture):
    rels, text, want, cases, lines, rows = _batch(fixture)
    _load_fixture(ctx, fixture)
    run = lambda t: ctx.run_theta(t)
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)
    assert ctx.last_result_rows() == rows[-1]
    for c, r in list(zip(cases, rows))[::5]:
        run(c["input"])
        assert ctx.last_result_rows() == r, c["input"]
    for q in _refused(fixture):                         # the batch ends with the lines before it
        assert run(cases[0]["input"] + q + cases[0]["input"]) == (lines[0], lib.QE_ENOTSUP)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("fixture", list(tt.CORPUS))
def test_theta_batch_on_local_ranks_is_truth(ctx, fixture, nranks):
    rels, text, want, cases, lines, _ = _batch(fixture)
    _load_fixture(ctx, fixture)
    run = lambda t: ctx.run_theta_local(t, nranks)[:2]
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)
    for q in _refused(fixture):                         # every rank leaves together
        assert run(cases[0]["input"] + q + cases[0]["input"]) == (lines[0], lib.QE_ENOTSUP)


@pytest.mark.parametrize("fixture", list(tt.CORPUS))
def test_theta_batch_on_lanes_is_truth(ctx, fixture):
    rels, text, want, cases, lines, _ = _batch(fixture)
    _load_fixture(ctx, fixture)
    run = lambda t: ctx.run_lanes(t, 4, executor=lib.QE_EXEC_THETA)
    if run(text) != (want, 0):
        _explain(run, cases, lines)
    assert run(text) == (want, 0)
    assert ctx.run_lanes(text, 1, executor=lib.QE_EXEC_THETA) == (want, 0)


def _binary(paths, queries, env):
    r = subprocess.run([QUERIES], input=dg.protocol_input(paths, queries).encode(), capture_output=True, timeout=600,
                       env=dict(os.environ, QE_RELATIONAL="2", **env))
    return r.stdout.decode("latin-1"), r.returncode


@pytest.mark.parametrize("env", [{}, {"QE_LOCAL_RANKS": "2"}], ids=["plain", "local2"])
@pytest.mark.parametrize("fixture", list(tt.CORPUS))
def test_binary_theta_mode(fixture, env):
    doc = goldens.load(f"{goldens.GOLDEN_DIR}/{fixture}.json")
    _, paths = goldens.dataset(doc["dataset"])
    _, text, want, cases, lines, _ = _batch(fixture)
    assert _binary(paths, text, env) == (want, 0)
    for q in _refused(fixture):
        assert _binary(paths, cases[0]["input"] + q + cases[0]["input"], env) == (lines[0], 70)


def test_queries_without_an_inequality_print_the_relational_lines(ctx):
    for fixture in rt.CORPUS:
        _, cases, want = rt.corpus(fixture)
        _load_fixture(ctx, fixture)
        text = "".join(c["input"] for c in cases[::4])
        got = ctx.run_theta(text)
        assert got == ctx.run_relational(text)
        assert got == ("".join(want[::4]), 0)


def test_a_link_side_may_be_filtered_to_nothing_on_a_rank(ctx):
    """hand-written shapes on fuzz_b: NULL links, a link beside an unlinked component, b.x < b.x"""
    _load_fixture(ctx, "fuzz_b")
    rels, _, _ = rt.corpus("fuzz_b")
    for q in ("0 1|0.0<1.0|0.1 1.1\n", "0 1 2|0.0=1.0&1.1>2.1|0.2 1.2 2.2\n", "0 1 2|0.0<1.0|0.1 1.1 2.1\n",
              "0 1|0.0<1.0&0.0>4000000000|0.1\n", "0 1|0.0>1.0&0.0<5|0.1 1.2\n", "0|0.1<0.1|0.0\n",
              "0 1|0.0=1.0&0.1<1.1|0.2 1.2\n"):
        want = tt.evaluate(q, rels)
        assert ctx.run_theta(q) == (want, 0), q
        assert ctx.last_result_rows() == tt.total_rows(q, rels), q
        assert ctx.run_theta_local(q, 3)[:2] == (want, 0), q
    for q in ("0 1 2|0.0<1.0&1.1<2.1|0.1\n", "0 1|0.0<1.0&0.1>1.1|0.1\n"):     # a chain, a band
        assert ctx.run_theta(q) == ("", lib.QE_ENOTSUP)
        assert ctx.run_theta_local(q, 2)[:2] == ("", lib.QE_ENOTSUP)
    assert ctx.run_relational("0 1|0.0<1.0|0.1\n") == ("", lib.QE_ENOTSUP)      # the plain mode keeps refusing


def test_stage_accounting(ctx):
    """theta_counts launches for a link query, none for an equality-only batch"""
    _load_fixture(ctx, "fuzz_b")
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        assert ctx.run_theta("0 1|0.0<1.0|0.1 1.1\n")[1] == 0
        st = ctx.kernel_stats()
        assert st["theta_counts"]["launches"] == 2      # one pass per side of the link
        rels, _, _ = rt.corpus("fuzz_b")
        n0, n1 = len(rels[0][0]), len(rels[1][0])       # 8 nR + 8 nS + 4 nR per pass
        assert st["theta_counts"]["alg_bytes"] == 20 * (n0 + n1)
        assert st["checksum_weighted"]["launches"] == 2
        ctx.reset_stats()
        assert ctx.run_theta("0 1|0.0=1.0&0.1<1.1|0.2 1.2\n")[1] == 0
        st = ctx.kernel_stats()
        assert st["select_compare"]["launches"] >= 1
        assert st.get("theta_counts", {}).get("launches", 0) == 0
        ctx.reset_stats()
        _, cases, _ = rt.corpus("fuzz_b")
        assert ctx.run_theta("".join(c["input"] for c in cases[::4]))[1] == 0
        st = ctx.kernel_stats()
        assert st.get("theta_counts", {}).get("launches", 0) == 0
        assert st.get("select_compare", {}).get("launches", 0) == 0
    finally:
        ctx.set_profiling(False)
