"""Theta-tree-mode truth in numpy: tests/theta_truth.py's semantics with the link rule widened to any
forest of links (include/qe_plan.h qe_plan_run_text_theta_tree).  TEST
INFRASTRUCTURE ONLY.

The < / > predicates between two groups of bindings are the edges of a graph over the joined
components.  A tree T of that graph counts as one component of P_T row tuples satisfying all its
links; a select of a binding of component x prints sum_i v_i * W_x(i), W_x(i) the number of such
tuples through row i, by message passing: W_x = prod_{y in N(x)} M_{y->x}, M_{y->x}(i) = sum_{j :
kx_i op ky_j} U_{y\\x}(j), U_{y\\x} = prod_{z in N(y), z != x} M_{z->y}.  Two links between one pair of
components (a band) and a cycle of links are refused: evaluate returns None.
tests/test_plan_theta_tree.py checks this evaluator against a brute-force nested-loop one.
"""
from __future__ import annotations

import os

import numpy as np

import goldens
import rel_truth as rt
import theta_truth as tt

M64 = rt.M64
CORPUS = tt.CORPUS


def link_forest(line: str):
    """the < / > predicates between two groups, or None when they hold a band or a cycle"""
    rels, cmps, _, _ = tt.parse(line)
    root = tt._groups(len(rels), cmps)
    tree = list(range(len(rels)))
    links, seen = [], set()
    for p in cmps:
        b1, _, op, b2, _ = p
        a, b = root[b1], root[b2]
        if op == "=" or a == b:
            continue
        if frozenset((a, b)) in seen or tt._find(tree, a) == tt._find(tree, b):
            return None
        seen.add(frozenset((a, b)))
        tree[tt._find(tree, a)] = tt._find(tree, b)
        links.append(p)
    return links


def message(kx: np.ndarray, ky: np.ndarray, u: np.ndarray, op: str) -> np.ndarray:
    """M[i] = sum_{j : kx[i] op ky[j]} u[j] mod 2^64"""
    order = np.argsort(ky, kind="stable")
    ks = ky[order]
    with np.errstate(over="ignore"):
        pre = np.concatenate([np.zeros(1, np.uint64), np.cumsum(u[order], dtype=np.uint64)])
        if op == "<":
            return pre[-1] - pre[np.searchsorted(ks, kx, "right")]
    return pre[np.searchsorted(ks, kx, "left")]


def _components(line: str, relations):
    """theta truth's components after filters, joins and selections: (comp, owner, col)"""
    rels, cmps, filters, _ = tt.parse(line)
    nb = len(rels)
    col = lambda b, c: relations[rels[b]][c]
    rows = {b: np.arange(len(col(b, 0)), dtype=np.int64) for b in range(nb)}
    for b, c, op, v in filters:
        rows[b] = rows[b][tt._cmp(col(b, c)[rows[b]], op, np.uint64(v))]
    for b1, c1, op, b2, c2 in cmps:
        if b1 == b2:
            rows[b1] = rows[b1][tt._cmp(col(b1, c1)[rows[b1]], op, col(b1, c2)[rows[b1]])]
    comp = {b: {b: rows[b]} for b in range(nb)}
    owner = list(range(nb))
    for b1, c1, op, b2, c2 in cmps:
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
    for b1, c1, op, b2, c2 in cmps:
        if op == "=" or b1 == b2 or owner[b1] != owner[b2]:
            continue
        o = owner[b1]
        keep = tt._cmp(col(b1, c1)[comp[o][b1]], op, col(b2, c2)[comp[o][b2]])
        comp[o] = {b: r[keep] for b, r in comp[o].items()}
    return comp, owner, col


def _evaluate(line: str, relations):
    """(select strings, total) or None"""
    links = link_forest(line)
    if links is None:
        return None
    _, _, _, sels = tt.parse(line)
    comp, owner, col = _components(line, relations)
    size = {o: len(next(iter(c.values()))) for o, c in comp.items()}
    # the forest: adj[x] = [(y, kx, ky, op as seen from x)]
    adj = {o: [] for o in comp}
    flip = {"<": ">", ">": "<"}
    for b1, c1, op, b2, c2 in links:
        o1, o2 = owner[b1], owner[b2]
        k1, k2 = col(b1, c1)[comp[o1][b1]], col(b2, c2)[comp[o2][b2]]
        adj[o1].append((o2, k1, k2, op))
        adj[o2].append((o1, k2, k1, flip[op]))

    def msg(y, x):
        """M_{y->x}, aligned with x's rows"""
        u = np.ones(size[y], dtype=np.uint64)
        for z, _, _, _ in adj[y]:
            if z != x:
                with np.errstate(over="ignore"):
                    u = u * msg(z, y)
        kx, ky, op = next((k1, k2, o) for n, k1, k2, o in adj[x] if n == y)
        return message(kx, ky, u, op)

    def weight(x):
        w = np.ones(size[x], dtype=np.uint64)
        for y, _, _, _ in adj[x]:
            with np.errstate(over="ignore"):
                w = w * msg(y, x)
        return w

    tree, trees = {}, []
    for o in comp:                                       # a tree per linked component, flooded
        if o in tree or not adj[o]:
            continue
        tree[o] = len(trees)
        todo = [o]
        while todo:
            for y, _, _, _ in adj[todo.pop()]:
                if y not in tree:
                    tree[y] = len(trees)
                    todo.append(y)
        bound = 1
        for x, t in tree.items():
            if t == len(trees):
                bound *= size[x]
        assert bound < 1 << 64                           # the mode's exactness bound: messages are exact
        trees.append(int(weight(o).sum(dtype=np.uint64)))
    total = 1
    for o in comp:
        if o not in tree:
            total *= size[o]
    for p in trees:
        total *= p
    out = []
    for b, c in sels:
        if total == 0:
            out.append("NULL ")
            continue
        o = owner[b]
        v = col(b, c)[comp[o][b]]
        with np.errstate(over="ignore"):
            if o in tree:
                own = trees[tree[o]]
                s = int(np.sum(v * weight(o), dtype=np.uint64))
            else:
                own = size[o]
                s = int(np.sum(v, dtype=np.uint64))
        out.append(f"{(s * (total // own)) & M64} ")
    return "".join(out) + "\n", min(total, M64)


def evaluate(line: str, relations):
    """the line theta-tree mode prints, or None for a shape it refuses (QE_ENOTSUP)"""
    r = _evaluate(line, relations)
    return None if r is None else r[0]


def total_rows(line: str, relations):
    r = _evaluate(line, relations)
    return None if r is None else r[1]


_TRUTH: dict = {}


def corpus(fixture: str):
    """(relations, cases, truth lines, rows) of a fixture's column < / > column cases, once per process"""
    if fixture not in _TRUTH:
        doc = goldens.load(os.path.join(goldens.GOLDEN_DIR, f"{fixture}.json"))
        rels, _ = goldens.dataset(doc["dataset"])
        cases = tt.corpus_cases(fixture)
        ev = [_evaluate(c["input"], rels) for c in cases]
        _TRUTH[fixture] = (rels, cases, [None if r is None else r[0] for r in ev],
                           [None if r is None else r[1] for r in ev])
    return _TRUTH[fixture]
