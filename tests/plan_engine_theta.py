"""tests/plan_engine_rel.py's numpy (+ gloo) engine with the theta mode's four callbacks -- the
struct extended by qe_engine's last fields select_cmp, allgather, theta_weights and
checksums_weighted -- and the theta entry points of libqeplan.so (include/qe_plan.h).  TEST
INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import plan_engine as pe
import plan_engine_rel as per
from plan_engine import H, I, P, U32, U64, VP

SELECT_CMP = C.CFUNCTYPE(I, VP, U32, U32, H, C.c_char, U32, U32, H, I, P(H), P(H))
ALLGATHER = C.CFUNCTYPE(I, VP, H, P(H))
THETA_WEIGHTS = C.CFUNCTYPE(I, VP, H, H, C.c_char, P(H), P(U64))
CHECKSUMS_WEIGHTED = C.CFUNCTYPE(I, VP, I, P(U32), P(U32), P(H), P(H), P(U64))
THETA_FIELDS = [("select_cmp", SELECT_CMP), ("allgather", ALLGATHER), ("theta_weights", THETA_WEIGHTS),
                ("checksums_weighted", CHECKSUMS_WEIGHTED)]


class EngineTheta(C.Structure):
    _fields_ = list(per.EngineRel._fields_) + THETA_FIELDS


class NumpyPlanEngineTheta(per.NumpyPlanEngineRel):
    def __init__(self, rels, rank=0, world=1, group=None, theta_callbacks=True, **opts):
        super().__init__(rels, rank, world, group, **opts)
        e = EngineTheta()
        C.memmove(C.byref(e), C.byref(self.e), C.sizeof(per.EngineRel))
        self._theta_cbs = []
        for name, ftype in THETA_FIELDS:
            if not theta_callbacks:
                continue                                 # NULL: the theta entry points return QE_EINVAL
            cb = ftype(self._wrap(getattr(self, "cb_" + name), False))
            self._theta_cbs.append(cb)
            setattr(e, name, cb)
        self.e = e
        self.select_cmp_calls = 0
        self.allgather_calls = 0
        self.theta_weights_calls = 0
        self.weighted_calls = 0
        for f in (self.lib.qe_plan_run_text, self.lib.qe_plan_check_text, self.lib.qe_plan_run_text_relational):
            f.argtypes = [P(EngineTheta)] + list(f.argtypes[1:])
        self.lib.qe_plan_run_text_theta.argtypes = [P(EngineTheta), C.c_char_p, P(C.c_void_p), P(C.c_size_t), P(U64)]

    def run_theta(self, text: str):
        """(stdout, rc, rows)"""
        out, n, rows = C.c_void_p(), C.c_size_t(), U64()
        rc = self.lib.qe_plan_run_text_theta(C.byref(self.e), text.encode(), C.byref(out), C.byref(n), C.byref(rows))
        s = C.string_at(out, n.value).decode("latin-1") if out.value else ""
        if out.value:
            self.libc.free(out)
        return s, rc, rows.value

    def why(self) -> str:
        return self.lib.qe_plan_why().decode()

    def cb_select_cmp(self, u, rel_a, col_a, a, op, rel_b, col_b, b, n, lists, outs):
        self.select_cmp_calls += 1
        keep = pe._OPS[op.decode()](self.rels[rel_a][col_a][self.get(a)], self.rels[rel_b][col_b][self.get(b)])
        for i in range(n):
            outs[i] = self.put(self.get(lists[i])[keep])

    def cb_allgather(self, u, keys, out):
        import torch
        import torch.distributed as dist
        assert self.world > 1                            # (the plan never calls it at one rank)
        self.allgather_calls += 1
        k = np.ascontiguousarray(self.get(keys))
        cnt = torch.tensor([len(k)], dtype=torch.int64)
        cnts = [torch.zeros(1, dtype=torch.int64) for _ in range(self.world)]
        dist.all_gather(cnts, cnt, group=self.group)
        cap = max(int(c) for c in cnts)
        mine = torch.zeros(cap, dtype=torch.int64)
        mine[:len(k)] = torch.from_numpy(k.view(np.int64).copy())
        parts = [torch.zeros(cap, dtype=torch.int64) for _ in range(self.world)]
        dist.all_gather(parts, mine, group=self.group)
        allk = np.concatenate([p.numpy()[:int(c)] for p, c in zip(parts, cnts)]).view(np.uint64)
        out[0] = self.put(allk)

    def cb_theta_weights(self, u, qk, sk, op, w, pairs):
        self.theta_weights_calls += 1
        k, s = self.get(qk), np.sort(self.get(sk))
        if len(k) >> 32 or len(s) >> 32:
            return -5
        if op.decode() == "<":
            cnt = len(s) - np.searchsorted(s, k, "right")
        else:
            cnt = np.searchsorted(s, k, "left")
        w[0] = self.put(cnt.astype(np.uint32))
        pairs[0] = int(cnt.sum())

    def cb_checksums_weighted(self, u, n, rels, cols, rows, w, sums):
        self.weighted_calls += 1
        for i in range(n):
            assert rels[i] != pe.VALUES
            v = self.rels[rels[i]][cols[i]][self.get(rows[i])]
            with np.errstate(over="ignore"):
                sums[i] = int(np.sum(v * self.get(w[i]).astype(np.uint64), dtype=np.uint64))


def worker(rank, world, port, rels, queries, outq, opts=None):
    """one gloo rank: every query through the theta mode, rank 0 reports ((stdout, rc, rows) per
    query, live handles, all-gathers made)"""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = NumpyPlanEngineTheta(rels, rank, world, **(opts or {}))
        res = [eng.run_theta(q) for q in queries]
        if rank == 0:
            outq.put((res, eng.live_handles(), eng.allgather_calls))
    finally:
        dist.destroy_process_group()
