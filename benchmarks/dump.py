"""bench.py --dump-outputs DIR: what the timed path handed its caller in the last timed step, as
.npy files two builds can be compared by.

Every executor behind bench.py returns the bytes the reference would print (row counts and u64
checksums as decimal text, `NULL` for an empty result) plus the result's row / pair count.  A u64
checksum does not fit a float64, so each printed number is stored as its two 32-bit halves, both
exact in float64:

    stdout_bytes.npy   float32 [len]   the printed bytes, one value (0..255) per byte
    values_hi32.npy    float64 [k]     every whitespace-separated token of the output, in order:
    values_lo32.npy    float64 [k]       value >> 32 and value & 0xffffffff (-1 / -1 for NULL)
    result_rows.npy    float64 [1]     the count `value` is made from: the executor's result rows (C3)
                                       or pairs (C5); C4: the batch's output lines
"""
from __future__ import annotations

import os

import numpy as np


def dump_outputs(directory: str, stdout: str, result_rows: int) -> None:
    os.makedirs(directory, exist_ok=True)
    raw = np.frombuffer(stdout.encode(), dtype=np.uint8)
    hi, lo = [], []
    for tok in stdout.split():
        v = int(tok) if tok.isdigit() else None
        hi.append(-1.0 if v is None else float(v >> 32))
        lo.append(-1.0 if v is None else float(v & 0xFFFFFFFF))
    np.save(os.path.join(directory, "stdout_bytes.npy"), raw.astype(np.float32))
    np.save(os.path.join(directory, "values_hi32.npy"), np.asarray(hi, dtype=np.float64))
    np.save(os.path.join(directory, "values_lo32.npy"), np.asarray(lo, dtype=np.float64))
    np.save(os.path.join(directory, "result_rows.npy"), np.asarray([float(result_rows)], dtype=np.float64))
