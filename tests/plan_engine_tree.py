"""tests/plan_engine_theta.py's numpy (+ gloo) engine with the theta-tree mode's two callbacks -- the
struct extended by qe_engine's last fields theta_wsums and checksums_weighted64 -- and the
theta-tree entry points of libqeplan.so (include/qe_plan.h).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import plan_engine as pe
import plan_engine_theta as pet
from plan_engine import H, I, P, U32, U64, VP

THETA_WSUMS = C.CFUNCTYPE(I, VP, H, H, H, C.c_char, H, P(H), P(U64))
CHECKSUMS_WEIGHTED64 = C.CFUNCTYPE(I, VP, I, P(U32), P(U32), P(H), P(H), P(U64))
TREE_FIELDS = [("theta_wsums", THETA_WSUMS), ("checksums_weighted64", CHECKSUMS_WEIGHTED64)]


class EngineTree(C.Structure):
    _fields_ = list(pet.EngineTheta._fields_) + TREE_FIELDS


class NumpyPlanEngineTree(pet.NumpyPlanEngineTheta):
    def __init__(self, rels, rank=0, world=1, group=None, theta_callbacks=True, tree_callbacks=True,
                 inflate_lengths=0, **opts):
        super().__init__(rels, rank, world, group, theta_callbacks=theta_callbacks, **opts)
        e = EngineTree()
        C.memmove(C.byref(e), C.byref(self.e), C.sizeof(pet.EngineTheta))
        self._tree_cbs = []
        for name, ftype in TREE_FIELDS:
            if not tree_callbacks:
                continue                                 # NULL: the theta-tree entry points return QE_EINVAL
            cb = ftype(self._wrap(getattr(self, "cb_" + name), False))
            self._tree_cbs.append(cb)
            setattr(e, name, cb)
        self.e = e
        self.wsums_calls = 0
        self.wsums_weighted_calls = 0                    # ... of them with far-side weights
        self.weighted64_calls = 0
        for f in (self.lib.qe_plan_run_text, self.lib.qe_plan_check_text, self.lib.qe_plan_run_text_relational,
                  self.lib.qe_plan_run_text_theta):
            f.argtypes = [P(EngineTree)] + list(f.argtypes[1:])
        self.lib.qe_plan_run_text_theta_tree.argtypes = [P(EngineTree), C.c_char_p, P(C.c_void_p), P(C.c_size_t),
                                                         P(U64)]
        if inflate_lengths:
            # every list reports `inflate_lengths` times its length: sizes beyond anything allocatable,
            # for the exactness bound (the arrays themselves stay small)
            self._length_cb = type(self.e.length)(
                self._wrap(lambda u, h, n: n.__setitem__(0, len(self.get(h)) * inflate_lengths), False))
            self.e.length = self._length_cb

    def run_theta_tree(self, text: str):
        """(stdout, rc, rows)"""
        out, n, rows = C.c_void_p(), C.c_size_t(), U64()
        rc = self.lib.qe_plan_run_text_theta_tree(C.byref(self.e), text.encode(), C.byref(out), C.byref(n),
                                                  C.byref(rows))
        s = C.string_at(out, n.value).decode("latin-1") if out.value else ""
        if out.value:
            self.libc.free(out)
        return s, rc, rows.value

    def cb_theta_wsums(self, u, qk, sk, sw, op, mul, out, total):
        self.wsums_calls += 1
        self.wsums_weighted_calls += bool(sw)
        k, s = self.get(qk), self.get(sk)
        if len(k) >> 32 or len(s) >> 32:
            return -5
        w = self.get(sw) if sw else np.ones(len(s), dtype=np.uint64)
        assert w.dtype == np.uint64 and len(w) == len(s)
        order = np.argsort(s, kind="stable")
        ks = s[order]
        with np.errstate(over="ignore"):
            pre = np.concatenate([np.zeros(1, np.uint64), np.cumsum(w[order], dtype=np.uint64)])
            if op.decode() == "<":
                m = pre[-1] - pre[np.searchsorted(ks, k, "right")]
            else:
                m = pre[np.searchsorted(ks, k, "left")]
            if mul:
                assert self.get(mul).dtype == np.uint64 and len(self.get(mul)) == len(k)
                m = m * self.get(mul)
            out[0] = self.put(m.astype(np.uint64))
            total[0] = int(np.sum(m, dtype=np.uint64))

    def cb_checksums_weighted64(self, u, n, rels, cols, rows, w, sums):
        self.weighted64_calls += 1
        for i in range(n):
            assert rels[i] != pe.VALUES and self.get(w[i]).dtype == np.uint64
            v = self.rels[rels[i]][cols[i]][self.get(rows[i])]
            with np.errstate(over="ignore"):
                sums[i] = int(np.sum(v * self.get(w[i]), dtype=np.uint64))


def worker(rank, world, port, rels, queries, outq, opts=None):
    """one gloo rank: every query through the theta-tree mode, rank 0 reports ((stdout, rc, rows) per
    query, live handles, all-gathers made, theta_wsums calls)"""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = NumpyPlanEngineTree(rels, rank, world, **(opts or {}))
        res = [eng.run_theta_tree(q) for q in queries]
        if rank == 0:
            outq.put((res, eng.live_handles(), eng.allgather_calls, eng.wsums_calls))
    finally:
        dist.destroy_process_group()
