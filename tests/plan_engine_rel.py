"""tests/plan_engine.py's numpy (+ gloo) engine with the relational mode's callback: the struct
extended by qe_engine's last field, select_eq, and the relational entry points of libqeplan.so
(include/qe_plan.h).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import plan_engine as pe
from plan_engine import H, I, P, U32, U64, VP

SELECT_EQ = C.CFUNCTYPE(I, VP, U32, U32, H, U32, U32, H, I, P(H), P(H))


class EngineRel(C.Structure):
    _fields_ = list(pe.Engine._fields_) + [("select_eq", SELECT_EQ)]


class NumpyPlanEngineRel(pe.NumpyPlanEngine):
    def __init__(self, rels, rank=0, world=1, group=None, **opts):
        super().__init__(rels, rank, world, group, **opts)
        e = EngineRel()
        C.memmove(C.byref(e), C.byref(self.e), C.sizeof(pe.Engine))     # the base engine's callbacks
        self._sel_cb = SELECT_EQ(self._wrap(self.cb_select_eq, False))
        e.select_eq = self._sel_cb
        self.e = e
        self.select_eq_calls = 0
        self.select_eq_lists = 0                 # the widest component a selection compacted
        for f in (self.lib.qe_plan_run_text, self.lib.qe_plan_check_text):    # (they read the struct's head only)
            f.argtypes = [P(EngineRel)] + list(f.argtypes[1:])
        self.lib.qe_plan_run_text_relational.argtypes = [P(EngineRel), C.c_char_p, P(C.c_void_p), P(C.c_size_t),
                                                         P(U64)]

    def run_relational(self, text: str):
        """(stdout, rc, rows)"""
        out, n, rows = C.c_void_p(), C.c_size_t(), U64()
        rc = self.lib.qe_plan_run_text_relational(C.byref(self.e), text.encode(), C.byref(out), C.byref(n),
                                                  C.byref(rows))
        s = C.string_at(out, n.value).decode("latin-1") if out.value else ""
        if out.value:
            self.libc.free(out)
        return s, rc, rows.value

    def cb_select_eq(self, u, rel_a, col_a, a, rel_b, col_b, b, n, lists, outs):
        self.select_eq_calls += 1
        self.select_eq_lists = max(self.select_eq_lists, n)
        keep = self.rels[rel_a][col_a][self.get(a)] == self.rels[rel_b][col_b][self.get(b)]
        for i in range(n):
            outs[i] = self.put(self.get(lists[i])[keep])


def worker(rank, world, port, rels, queries, outq, opts=None):
    """one gloo rank: every query through the relational mode, rank 0 reports ((stdout, rc, rows) per
    query, live handles)"""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = NumpyPlanEngineRel(rels, rank, world, **(opts or {}))
        res = [eng.run_relational(q) for q in queries]
        if rank == 0:
            outq.put((res, eng.live_handles()))
    finally:
        dist.destroy_process_group()
