"""The theta-tree mode on the GPU: qe_theta_wsums and qe_checksum_weighted64 against numpy, and
qe_run_queries_theta_tree -- one rank, in-process ranks, the lanes and the `queries` binary -- against
theta-tree truth (tests/tree_truth.py) on the hand-written chains, stars and trees of
tests/test_plan_theta_tree.py and on the 68 corpus cases with a column < / > column predicate."""
import json
import os
import subprocess

import numpy as np
import pytest

import goldens
import rel_truth as rt
import test_gpu_theta as tgt
import test_plan_theta as tpt
import test_plan_theta_tree as tptt
import theta_truth as tt
import tree_truth as trt
from qe import datagen as dg
from qe import lib

pytestmark = pytest.mark.gpu

QUERIES = tgt.QUERIES
MJ_TILE = tgt.MJ_TILE
SCAN_ONE_BLOCK = 32768                                  # the gather-scan's single-block / chunked boundary
_loaded = {"key": None}


def _load(ctx, key, rels):
    if _loaded["key"] != key:
        ctx.drop_relations()
        for cols in rels():
            ctx.load_relation(cols)
        _loaded["key"] = key


def _load_fixture(ctx, fixture):
    ds = goldens.load(f"{goldens.GOLDEN_DIR}/{fixture}.json")["dataset"]
    _load(ctx, json.dumps(ds, sort_keys=True), lambda: goldens.dataset(ds)[0])


def _load_small(ctx):
    _load(ctx, "small", tpt._small)


# ---- qe_theta_wsums -----------------------------------------------------------------------------

def _reference(rs, rval, ss, sval, sw, op, mul):
    """stable argsort (the sides arrive sorted), cumsum in uint64, searchsorted"""
    w = np.ones(len(ss), np.uint64) if sw is None else sw[sval]
    with np.errstate(over="ignore"):
        pre = np.concatenate([np.zeros(1, np.uint64), np.cumsum(w, dtype=np.uint64)])
        if op == "<":
            m = pre[-1] - pre[np.searchsorted(ss, rs, "right")]
        else:
            m = pre[np.searchsorted(ss, rs, "left")]
        out = np.zeros(len(rs), np.uint64)
        out[rval] = m
        if mul is not None:
            out = out * mul
        return out, int(np.sum(out, dtype=np.uint64))


@pytest.mark.parametrize("pattern", ["equal", "single", "dups", "wide"])
def test_theta_wsums_against_numpy(ctx, pattern):
    rng = np.random.default_rng(21)
    full = lambda n: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    for nS in (0, 1, 8195, SCAN_ONE_BLOCK, SCAN_ONE_BLOCK + 1):
        for nR in (1, MJ_TILE - 1, MJ_TILE, MJ_TILE + 1, 3 * MJ_TILE + 5):
            rk, sk = tgt._keys(pattern, nR, nS, rng)
            order_r, order_s = np.argsort(rk, kind="stable"), np.argsort(sk, kind="stable")
            rs, ss = rk[order_r], sk[order_s]
            rval, sval = rng.permutation(nR).astype(np.uint32), rng.permutation(nS).astype(np.uint32)
            R, S = ctx.pairs_from_host(rs, rval), ctx.pairs_from_host(ss, sval)
            R.flags |= lib.PAIRS_SORTED
            S.flags |= lib.PAIRS_SORTED
            weights = {"null": None, "ones": np.ones(nS, np.uint64), "zeros": np.zeros(nS, np.uint64),
                       "random": full(nS)}                  # (full 64-bit: the sums wrap)
            mulh = full(nR)
            d_mul, d_out = ctx.u64_from_host(mulh), ctx.u64_from_host(np.full(nR, 0xDEAD, np.uint64))
            for kind, sw in weights.items():
                d_sw = ctx.u64_from_host(sw) if sw is not None else None
                for op in "<>":
                    for mul in (None, mulh):
                        want, total = _reference(rs, rval, ss, sval, sw, op, mul)
                        got_total = ctx.theta_wsums(R, S, d_sw, op, d_mul if mul is not None else None, d_out)
                        got = ctx.u64_to_host(d_out, nR)
                        where = (pattern, nR, nS, kind, op, mul is not None)
                        assert np.array_equal(got, want), where
                        assert got_total == total, where
                        if kind in ("null", "ones") and mul is None:    # theta_counts' counts
                            counts = np.zeros(nR, np.uint64)
                            counts[rval] = tt.weights(rs, ss, op)
                            assert np.array_equal(got, counts), where
                        if kind == "zeros" or pattern == "equal":
                            assert got_total == 0 and not got.any(), where
                if d_sw is not None:
                    ctx.buffer_free(d_sw)
            if nS == 8195 and nR == MJ_TILE + 1:            # ... and qe_theta_counts itself agrees
                pairs = ctx.theta_counts(R, S, "<")
                assert pairs == ctx.theta_wsums(R, S, None, "<", None, d_out)
                counts = np.zeros(nR, np.uint64)
                counts[rval] = ctx.counts_to_host(R.match, nR)
                assert np.array_equal(ctx.u64_to_host(d_out, nR), counts)
            for d in (d_mul, d_out):
                ctx.buffer_free(d)
            ctx.pairs_free(R)
            ctx.pairs_free(S)


def test_theta_wsums_refuses_what_theta_counts_refuses(ctx):
    rng = np.random.default_rng(22)
    k = np.sort(rng.integers(0, 500, 1000).astype(np.uint64))
    val = np.arange(1000, dtype=np.uint32)
    R, S, U = (ctx.pairs_from_host(k, val) for _ in range(3))
    R.flags |= lib.PAIRS_SORTED
    S.flags |= lib.PAIRS_SORTED
    d_out = ctx.u64_from_host(np.zeros(1000, np.uint64))
    for bad in (lambda: ctx.theta_wsums(U, S, None, "<", None, d_out),
                lambda: ctx.theta_wsums(R, U, None, ">", None, d_out),
                lambda: ctx.theta_wsums(R, S, None, "=", None, d_out)):
        with pytest.raises(lib.QEError) as e:
            bad()
        assert e.value.code == lib.QE_EINVAL
    assert ctx.theta_wsums(R, S, None, "<", None, d_out) == int(tt.weights(k, k, "<").sum())
    ctx.buffer_free(d_out)
    for p in (R, S, U):
        ctx.pairs_free(p)


# ---- qe_checksum_weighted64 ---------------------------------------------------------------------

def test_checksum_weighted64_against_numpy(ctx):
    rng = np.random.default_rng(23)
    rows = 20_011
    col = rng.integers(0, 1 << 63, rows, dtype=np.uint64)
    ctx.drop_relations()
    _loaded["key"] = None
    rel = ctx.load_relation([col])
    block = 4 * 256 * 16                                    # one workgroup's stride of the kernel's grid
    for n in (0, 1, block - 1, block + 1):
        r = rng.integers(0, rows, n).astype(np.uint32)
        w = rng.integers(1 << 32, 1 << 63, n, dtype=np.uint64) * np.uint64(2)    # weights above 2^32
        if n > 1:
            w[1] = 0
        l, d_w = ctx.list_from_host(r), ctx.u64_from_host(w)
        with np.errstate(over="ignore"):
            want = int(np.sum(col[r] * w, dtype=np.uint64))
        assert ctx.checksum_weighted64(ctx.column(rel, 0), l, d_w) == want, n
        ctx.list_free(l)
        ctx.buffer_free(d_w)
    w = rng.integers(0, 1 << 63, rows, dtype=np.uint64)     # rows None: every row of the column
    d_w = ctx.u64_from_host(w)
    with np.errstate(over="ignore"):
        assert ctx.checksum_weighted64(ctx.column(rel, 0), None, d_w) == int(np.sum(col * w, dtype=np.uint64))
    ctx.buffer_free(d_w)


# ---- the executor -------------------------------------------------------------------------------

def _batch(fixture):
    """every inequality case of the fixture as one batch: the mode refuses none of them"""
    rels, cases, want, rows = trt.corpus(fixture)
    assert len(cases) == trt.CORPUS[fixture] and all(w is not None for w in want)
    return "".join(c["input"] for c in cases), "".join(want), cases, want, rows


def _hand():
    rels = tpt._small()
    table = [q + "\n" for q, _ in tptt.HAND + tpt.REFUSED[:2]]
    want = [trt.evaluate(q, rels) for q in table]
    assert sum(w.startswith("NULL") for w in want) == tptt.NULLS
    return table, want, [trt.total_rows(q, rels) for q in table]


def _explain(run, queries, want):
    """the first query that differs, run on its own (a batch's bytes do not say which line is wrong)"""
    for q, w in zip(queries, want):
        assert run(q) == (w, 0), q


def _check(run, queries, want):
    text, bytes_ = "".join(queries), "".join(want)
    if run(text) != (bytes_, 0):
        _explain(run, queries, want)
    assert run(text) == (bytes_, 0)


BAND = tptt.BANDS[0][0] + "\n"


def test_hand_written_shapes_are_truth(ctx):
    table, want, rows = _hand()
    _load_small(ctx)
    _check(lambda t: ctx.run_theta_tree(t), table, want)
    for q, r in list(zip(table, rows))[::3]:
        ctx.run_theta_tree(q)
        assert ctx.last_result_rows() == r, q
    for nranks in (2, 3):
        _check(lambda t: ctx.run_theta_tree_local(t, nranks)[:2], table, want)
    for workers in (4, 1):
        _check(lambda t: ctx.run_lanes(t, workers, executor=lib.QE_EXEC_THETA_TREE), table, want)
    # a band in the middle of a batch: the lines before it, then QE_ENOTSUP -- on every path
    cut = (want[0], lib.QE_ENOTSUP)
    text = table[0] + BAND + table[0]
    assert ctx.run_theta_tree(text) == cut
    assert ctx.run_theta_tree_local(text, 2)[:2] == cut
    assert ctx.run_lanes(text, 4, executor=lib.QE_EXEC_THETA_TREE) == cut
    assert ctx.run_theta_tree(tptt.CYCLE + "\n") == ("", lib.QE_ENOTSUP)
    assert ctx.run_theta(table[0]) == ("", lib.QE_ENOTSUP)     # theta mode keeps refusing the chain


@pytest.mark.parametrize("fixture", list(trt.CORPUS))
def test_corpus_batch_is_truth(ctx, fixture):
    text, want, cases, lines, rows = _batch(fixture)
    _load_fixture(ctx, fixture)
    queries = [c["input"] for c in cases]
    _check(lambda t: ctx.run_theta_tree(t), queries, lines)
    assert ctx.last_result_rows() == rows[-1]
    for q, r in list(zip(queries, rows))[::5]:
        ctx.run_theta_tree(q)
        assert ctx.last_result_rows() == r, q
    for q, r in zip(queries, rows):                         # the shape theta mode refuses: its pair count
        if r == tptt.FORMERLY_REFUSED.get(fixture):
            assert ctx.run_theta_tree(q)[1] == 0 and ctx.last_result_rows() == r
            assert ctx.run_theta(q) == ("", lib.QE_ENOTSUP)
    for nranks in (2, 3):
        _check(lambda t: ctx.run_theta_tree_local(t, nranks)[:2], queries, lines)
    for workers in (4, 1):
        _check(lambda t: ctx.run_lanes(t, workers, executor=lib.QE_EXEC_THETA_TREE), queries, lines)


def _binary(paths, queries, env):
    r = subprocess.run([QUERIES], input=dg.protocol_input(paths, queries).encode(), capture_output=True, timeout=600,
                       env=dict(os.environ, QE_RELATIONAL="3", **env))
    return r.stdout.decode("latin-1"), r.returncode


@pytest.mark.parametrize("env", [{}, {"QE_LOCAL_RANKS": "2"}], ids=["plain", "local2"])
def test_binary_theta_tree_mode(tmp_path, env):
    for fixture in trt.CORPUS:
        doc = goldens.load(f"{goldens.GOLDEN_DIR}/{fixture}.json")
        _, paths = goldens.dataset(doc["dataset"])
        text, want, _, _, _ = _batch(fixture)
        assert _binary(paths, text, env) == (want, 0)
    table, want, _ = _hand()
    paths = dg.write_dataset(str(tmp_path), tpt._small())
    assert _binary(paths, "".join(table), env) == ("".join(want), 0)
    assert _binary(paths, table[0] + BAND + table[0], env) == (want[0], 70)


def test_queries_without_an_inequality_print_the_relational_lines(ctx):
    _, cases, want = rt.corpus("fuzz_b")
    _load_fixture(ctx, "fuzz_b")
    text = "".join(c["input"] for c in cases[::4])
    got = ctx.run_theta_tree(text)
    assert got == ctx.run_relational(text)
    assert got == ("".join(want[::4]), 0)


def test_stage_accounting(ctx):
    """theta_wsums launches once per message; its bytes are DESIGN.md section 11's formula"""
    _load_small(ctx)
    n0, n1, n2 = (len(r[0]) for r in tpt._small())
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        assert ctx.run_theta_tree("0 1 2|0.0<1.0&1.1<2.1|0.1\n")[1] == 0    # C -> B, then B -> A weighted
        st = ctx.kernel_stats()
        assert st["theta_wsums"]["launches"] == 2
        # per launch 20 nR + 8 nS, + 8 nR with far-side weights (the prefix sums read), + 8 nR with mul
        assert st["theta_wsums"]["alg_bytes"] == (20 * n1 + 8 * n2) + (20 * n0 + 8 * n1 + 8 * n0)
        # the gather-scan of B's weights, single block: 12 nS read + 8 (nS + 1) written
        assert st["theta_wsums_scan"]["launches"] == 1
        assert st["theta_wsums_scan"]["alg_bytes"] == 12 * n1 + 8 * (n1 + 1)
        assert st["checksum_weighted64"]["launches"] == 1
        assert st["checksum_weighted64"]["alg_bytes"] == 12 * n0
        assert st.get("theta_counts", {}).get("launches", 0) == 0
        ctx.reset_stats()
        assert ctx.run_theta_tree("0 1 2|0.0<1.0&1.1<2.1|1.1\n")[1] == 0    # A -> B, then C -> B through mul
        st = ctx.kernel_stats()
        assert st["theta_wsums"]["launches"] == 2
        assert st["theta_wsums"]["alg_bytes"] == (20 * n1 + 8 * n0) + (20 * n1 + 8 * n2 + 8 * n1)
        assert st.get("theta_wsums_scan", {}).get("launches", 0) == 0
        ctx.reset_stats()
        assert ctx.run_theta_tree("0 1 2|0.0<1.0&1.1<2.1|0.1 2.1\n")[1] == 0
        assert ctx.kernel_stats()["theta_wsums"]["launches"] == 4
        ctx.reset_stats()
        assert ctx.run_theta_tree("0 1 2|0.0=1.0&1.1=2.1|0.1 2.1\n0 1|0.0=1.0&0.1<1.1|0.2\n")[1] == 0
        st = ctx.kernel_stats()
        for stage in ("theta_wsums", "theta_wsums_scan", "checksum_weighted64", "theta_counts"):
            assert st.get(stage, {}).get("launches", 0) == 0, stage
    finally:
        ctx.set_profiling(False)
