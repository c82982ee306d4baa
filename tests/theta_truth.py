"""Theta-mode truth in numpy: tests/rel_truth.py's semantics with a written column < / > column
predicate honoured (include/qe_plan.h qe_plan_run_text_theta).  TEST
INFRASTRUCTURE ONLY.

Comparisons are unsigned 64-bit and strict.  A predicate on one binding is a filter on its rows.
Bindings are grouped by union-find over the query's column = column predicates: a < / > predicate
inside a group is a selection on the joined component; one between two groups is a theta link --
the pair counts as one component of P = #{(i, j) : kA_i op kB_j} rows, a select of a binding of A
prints sum_i v_i * #{j : kA_i op kB_j} (B alike), nothing is materialised.  A group with two or
more links (a chain, a tree, a band between one pair) is refused: evaluate returns None.
tests/test_plan_theta.py checks this evaluator against a brute-force nested-loop one.
"""
from __future__ import annotations

import os

import numpy as np

import goldens
import rel_truth as rt

M64 = rt.M64
CORPUS = {"fuzz_a": 29, "fuzz_b": 17, "fuzz_c": 22}      # the single-query cases with such a predicate


def parse(line: str):
    """(relation ids, [(b1, c1, op, b2, c2)], [(b, c, op, v)], selects)"""
    rels_s, preds_s, sel_s = line.strip().split("|")
    rels = [int(x) for x in rels_s.split(" ")]
    cmps, filters = [], []
    for p in preds_s.split("&"):
        m = rt._JOIN.fullmatch(p)
        if m:
            a, b, op, c, d = m.groups()
            cmps.append((int(a), int(b), op, int(c), int(d)))
            continue
        a, b, op, c = rt._FILTER.fullmatch(p).groups()
        filters.append((int(a), int(b), op, int(c) & 0xFFFFFFFF))    # the reference's %u
    sels = [tuple(int(v) for v in s.split(".")) for s in sel_s.split(" ")]
    return rels, cmps, filters, sels


def _cmp(x, op, y):
    return x == y if op == "=" else (x > y if op == ">" else x < y)


def _find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def _groups(nb, cmps):
    parent = list(range(nb))
    for b1, _, op, b2, _ in cmps:
        if op == "=":
            parent[_find(parent, b1)] = _find(parent, b2)
    return [_find(parent, b) for b in range(nb)]


def link_predicates(line: str):
    """the < / > predicates between two groups, or None when some group has two or more"""
    rels, cmps, _, _ = parse(line)
    root = _groups(len(rels), cmps)
    links, count = [], {}
    for p in cmps:
        b1, _, op, b2, _ = p
        if op == "=" or root[b1] == root[b2]:
            continue
        links.append(p)
        for r in (root[b1], root[b2]):
            count[r] = count.get(r, 0) + 1
    return None if any(v > 1 for v in count.values()) else links


def weights(k: np.ndarray, other: np.ndarray, op: str) -> np.ndarray:
    """w[i] = #{j : k[i] op other[j]}, op '<' or '>'"""
    s = np.sort(other)
    if op == "<":
        return (len(s) - np.searchsorted(s, k, "right")).astype(np.uint64)
    return np.searchsorted(s, k, "left").astype(np.uint64)


def _evaluate(line: str, relations):
    """(select strings, total) or None"""
    links = link_predicates(line)
    if links is None:
        return None
    rels, cmps, filters, sels = parse(line)
    nb = len(rels)
    col = lambda b, c: relations[rels[b]][c]
    rows = {b: np.arange(len(col(b, 0)), dtype=np.int64) for b in range(nb)}
    for b, c, op, v in filters:
        rows[b] = rows[b][_cmp(col(b, c)[rows[b]], op, np.uint64(v))]
    for b1, c1, op, b2, c2 in cmps:                      # one binding: a filter, before it joins
        if b1 == b2:
            rows[b1] = rows[b1][_cmp(col(b1, c1)[rows[b1]], op, col(b1, c2)[rows[b1]])]
    comp = {b: {b: rows[b]} for b in range(nb)}
    owner = list(range(nb))
    for b1, c1, op, b2, c2 in cmps:                      # the equi-joins, in written order
        if op != "=" or b1 == b2:
            continue
        o1, o2 = owner[b1], owner[b2]
        k1, k2 = col(b1, c1)[comp[o1][b1]], col(b2, c2)[comp[o2][b2]]
        if o1 == o2:
            keep = k1 == k2
            comp[o1] = {b: r[keep] for b, r in comp[o1].items()}
            continue
        i1, i2 = rt._match(k1, k2)
        merged = {b: r[i1] for b, r in comp[o1].items()}
        merged.update({b: r[i2] for b, r in comp[o2].items()})
        comp[o1] = merged
        del comp[o2]
        owner = [o1 if o == o2 else o for o in owner]
    for b1, c1, op, b2, c2 in cmps:                      # < / > inside a component: a selection
        if op == "=" or b1 == b2 or owner[b1] != owner[b2]:
            continue
        o = owner[b1]
        keep = _cmp(col(b1, c1)[comp[o][b1]], op, col(b2, c2)[comp[o][b2]])
        comp[o] = {b: r[keep] for b, r in comp[o].items()}
    size = {r: len(next(iter(c.values()))) for r, c in comp.items()}
    w, partner = {}, {}
    for b1, c1, op, b2, c2 in links:                     # a link: weights, the pair is one component of P
        o1, o2 = owner[b1], owner[b2]
        k1, k2 = col(b1, c1)[comp[o1][b1]], col(b2, c2)[comp[o2][b2]]
        w[o1] = weights(k1, k2, op)
        w[o2] = weights(k2, k1, "<" if op == ">" else ">")
        partner[o1], partner[o2] = o2, o1
        size[o1] = int(w[o1].sum())                      # P, counted once: on the first side
        assert size[o1] == int(w[o2].sum())
        size[o2] = None
    total = 1
    for s in size.values():
        if s is not None:
            total *= s
    out = []
    for b, c in sels:
        if total == 0:
            out.append("NULL ")
            continue
        o = owner[b]
        v = col(b, c)[comp[o][b]]
        if o in w:
            own = size[o] if size[o] is not None else size[partner[o]]
            with np.errstate(over="ignore"):
                s = int(np.sum(v * w[o], dtype=np.uint64))   # (mod 2^64, like the printed number)
        else:
            own = size[o]
            s = int(np.sum(v, dtype=np.uint64))
        out.append(f"{(s * (total // own)) & M64} ")
    return "".join(out) + "\n", min(total, M64)


def evaluate(line: str, relations):
    """the line theta mode prints, or None for a shape it refuses (QE_ENOTSUP)"""
    r = _evaluate(line, relations)
    return None if r is None else r[0]


def total_rows(line: str, relations):
    r = _evaluate(line, relations)
    return None if r is None else r[1]


def corpus_cases(fixture: str) -> list[dict]:
    """the fixture's well-formed single-query cases with a column < or > column predicate, in file order"""
    doc = goldens.load(os.path.join(goldens.GOLDEN_DIR, f"{fixture}.json"))
    return [c for c in doc["cases"]
            if rt.WELL_FORMED.fullmatch(c["input"]) and rt.COLUMN_INEQUALITY.search(c["input"])]


_TRUTH: dict = {}


def corpus(fixture: str):
    """(relations, cases, truth lines (None: refused), rows) of a fixture, computed once per process"""
    if fixture not in _TRUTH:
        doc = goldens.load(os.path.join(goldens.GOLDEN_DIR, f"{fixture}.json"))
        rels, _ = goldens.dataset(doc["dataset"])
        cases = corpus_cases(fixture)
        ev = [_evaluate(c["input"], rels) for c in cases]
        _TRUTH[fixture] = (rels, cases, [None if r is None else r[0] for r in ev],
                           [None if r is None else r[1] for r in ev])
    return _TRUTH[fixture]
