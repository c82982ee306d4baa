"""Relational truth in numpy alone, with oracle/truth.py's semantics (which needs pandas; the GPU
machine may not have it): what the relational mode (include/qe_plan.h) must
print for a query line.  TEST INFRASTRUCTURE ONLY.

Filters first (they AND), then every column = column predicate in written order: an equi-join of two
components, or a selection inside one; the components that remain form a cross product, which is
never materialised -- a select prints its component's sum times the other components' sizes mod
2^64, or NULL when some component is empty.  tests/test_plan_relational.py checks this evaluator
against oracle/truth.py on the whole corpus below.
"""
from __future__ import annotations

import os
import re

import numpy as np

import goldens

M64 = (1 << 64) - 1
_JOIN = re.compile(r"(\d+)\.(\d+)([=<>])(\d+)\.(\d+)")
_FILTER = re.compile(r"(\d+)\.(\d+)([=<>])(\d+)")
WELL_FORMED = re.compile(r"[0-9 ]+\|[0-9.=<>&]+\|[0-9. ]+\n")
COLUMN_INEQUALITY = re.compile(r"\d+\.\d+[<>]\d+\.\d+")

# the fixtures whose single-query cases form the corpus, and how many of each run (every one but
# those with a column < or > column predicate, which the relational mode refuses)
CORPUS = {"fuzz_a": 194, "fuzz_b": 153, "fuzz_c": 149, "known_answers": 7}

# hand-written shapes on fuzz_b's dataset: (query, expected line, shape); expected with oracle/truth.py
HAND = [
    ("0|0.0=0.1|0.2", "3929831001 ", "same binding, two columns"),
    ("0|0.1=0.2|0.0", "NULL ", "same binding, no match"),
    ("1|0.0=0.0|0.1", "1464231 ", "no-op predicate"),
    ("0 1|0.0<1000|0.1 1.1", "1486233000 1453981383 ", "cross product with an unjoined binding"),
    ("0 1 2|0.0=1.0|0.1 2.1", "4609191000 4403406330 ", "select from an untouched binding"),
    ("0 1 2 3|0.0=1.0&2.0=3.0|0.1 3.1", "4544662326 4354810530 ", "two components"),
    ("0 1 2|0.0=1.0&1.0=2.0&0.0=2.0|0.1 2.2", "1511352 6306247727197 ", "triangle, redundant third predicate"),
    ("0 1 2|0.0=1.0&1.0=2.0&0.1=2.1|0.1 2.2", "1992 8280459384 ", "in-component predicate that filters"),
    ("0 1|0.0=1.0&0.1=1.1|0.2 1.2", "5010076349 4896438165 ", "two predicates between one pair"),
    ("0 1 2|0.0=1.0&0.2>2000000000&1.2<2000000000&2.2<1000000000&1.0=2.0|0.1 1.1 2.1", "102188 97253 97978 ",
     "filters on three bindings, written between the joins"),
    ("0 1|0.0=1.0&1.1=1.2|0.2", "NULL ", "in-component self-filter empties the join"),
]


def parse(line: str):
    rels_s, preds_s, sel_s = line.strip().split("|")
    rels = [int(x) for x in rels_s.split(" ")]
    joins, filters = [], []
    for p in preds_s.split("&"):
        m = _JOIN.fullmatch(p)
        if m:
            a, b, _, c, d = m.groups()
            joins.append((int(a), int(b), int(c), int(d)))
            continue
        a, b, op, c = _FILTER.fullmatch(p).groups()
        filters.append((int(a), int(b), op, int(c) & 0xFFFFFFFF))    # the reference's %u
    sels = [tuple(int(v) for v in s.split(".")) for s in sel_s.split(" ")]
    return rels, joins, filters, sels


def _match(ka: np.ndarray, kb: np.ndarray):
    """every (i, j) with ka[i] == kb[j]"""
    oa = np.argsort(ka, kind="stable")
    ob = np.argsort(kb, kind="stable")
    sa, sb = ka[oa], kb[ob]
    lo = np.searchsorted(sb, sa, "left")
    cnt = np.searchsorted(sb, sa, "right") - lo
    ia = np.repeat(oa, cnt)
    first = np.cumsum(cnt) - cnt                        # each a row's first pair
    jb = np.arange(int(cnt.sum())) - np.repeat(first, cnt) + np.repeat(lo, cnt)
    return ia, ob[jb]


def _components(line: str, relations):
    """(selects, column accessor, owner of each binding, root -> aligned rowid arrays by binding)"""
    rels, joins, filters, sels = parse(line)
    nb = len(rels)
    col = lambda b, c: relations[rels[b]][c]
    rows = {b: np.arange(len(col(b, 0)), dtype=np.int64) for b in range(nb)}
    for b, c, op, v in filters:
        x, v = col(b, c)[rows[b]], np.uint64(v)
        rows[b] = rows[b][x == v if op == "=" else (x > v if op == ">" else x < v)]
    comp = {b: {b: rows[b]} for b in range(nb)}
    owner = list(range(nb))
    for b1, c1, b2, c2 in joins:
        o1, o2 = owner[b1], owner[b2]
        k1, k2 = col(b1, c1)[comp[o1][b1]], col(b2, c2)[comp[o2][b2]]
        if o1 == o2:
            keep = k1 == k2
            comp[o1] = {b: r[keep] for b, r in comp[o1].items()}
            continue
        i1, i2 = _match(k1, k2)
        merged = {b: r[i1] for b, r in comp[o1].items()}
        merged.update({b: r[i2] for b, r in comp[o2].items()})
        comp[o1] = merged
        del comp[o2]
        owner = [o1 if o == o2 else o for o in owner]
    return sels, col, owner, comp


def evaluate(line: str, relations) -> str:
    sels, col, owner, comp = _components(line, relations)
    size = {r: len(next(iter(c.values()))) for r, c in comp.items()}
    total = 1
    for s in size.values():
        total *= s
    out = []
    for b, c in sels:
        if total == 0:
            out.append("NULL ")
            continue
        s = int(np.sum(col(b, c)[comp[owner[b]][b]], dtype=np.uint64))
        out.append(f"{(s * (total // size[owner[b]])) & M64} ")
    return "".join(out) + "\n"


def total_rows(line: str, relations) -> int:
    """the product of the component sizes (qe_last_result_rows in the relational mode), saturated"""
    total = 1
    for c in _components(line, relations)[3].values():
        total *= len(next(iter(c.values())))
    return min(total, M64)


def in_component(line: str) -> bool:
    """does some column = column predicate of the line run inside a component (both bindings
    already joined, or one binding's two columns)?"""
    rels, joins, _, _ = parse(line)
    owner = list(range(len(rels)))
    for b1, c1, b2, c2 in joins:
        if owner[b1] == owner[b2]:
            if (b1, c1) != (b2, c2):
                return True
            continue
        o1, o2 = owner[b1], owner[b2]
        owner = [o1 if o == o2 else o for o in owner]
    return False


def corpus_cases(fixture: str) -> list[dict]:
    """the fixture's single-query cases, in file order, without those the relational mode refuses
    (a column < or > column predicate)"""
    doc = goldens.load(os.path.join(goldens.GOLDEN_DIR, f"{fixture}.json"))
    return [c for c in doc["cases"]
            if WELL_FORMED.fullmatch(c["input"]) and not COLUMN_INEQUALITY.search(c["input"])]


_TRUTH: dict = {}


def corpus(fixture: str):
    """(relations, cases, truth lines) of a fixture, computed once per process"""
    if fixture not in _TRUTH:
        doc = goldens.load(os.path.join(goldens.GOLDEN_DIR, f"{fixture}.json"))
        rels, _ = goldens.dataset(doc["dataset"])
        cases = corpus_cases(fixture)
        _TRUTH[fixture] = (rels, cases, [evaluate(c["input"], rels) for c in cases])
    return _TRUTH[fixture]
