"""bench.py's plain run, `--full` and `--dump-outputs`.  CPU: the dump format (benchmarks/dump.py)
and the options through the launcher.  GPU: one small plain run and one small `--full` run of the
headline workload -- the plain line carries the headline figure alone, the dumped arrays are the
bytes the timed path printed, and `--full` still measures everything beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY_KEYS = ("roofline", "stages", "stage_roofline", "kernel_ms_per_step", "faithful_executor",
                  "materialised_last_join", "two_stream_sorts")
ROWS = 200_000          # several partition tiles per relation, a run of well under a second


def _env():
    return {k: v for k, v in os.environ.items()
            if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def _bench(args, timeout=170):
    p = subprocess.run([sys.executable, BENCH] + args, env=_env(), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout                   # one JSON result line
    return json.loads(lines[0])


def _u64(directory):
    hi = np.load(os.path.join(directory, "values_hi32.npy"))
    lo = np.load(os.path.join(directory, "values_lo32.npy"))
    assert hi.dtype == lo.dtype == np.float64
    return [None if h < 0 else (int(h) << 32) | int(l) for h, l in zip(hi, lo)]


def test_dump_outputs_is_exact_for_u64_checksums(tmp_path):
    from benchmarks.dump import dump_outputs
    text = "46567055\n100034367840717139 18446744073709551615 0 \nNULL 7\n"
    d = str(tmp_path / "nested" / "out")               # created on demand
    dump_outputs(d, text, 46567055)
    raw = np.load(os.path.join(d, "stdout_bytes.npy"))
    assert raw.dtype == np.float32
    assert bytes(raw.astype(np.uint8)).decode() == text
    assert _u64(d) == [46567055, 100034367840717139, 2**64 - 1, 0, None, 7]
    rows = np.load(os.path.join(d, "result_rows.npy"))
    assert rows.dtype == np.float64 and rows.tolist() == [46567055.0]
    assert sorted(os.listdir(d)) == ["result_rows.npy", "stdout_bytes.npy", "values_hi32.npy", "values_lo32.npy"]


def test_launcher_accepts_full_and_dump_outputs(tmp_path):
    d = _bench(["--gpus", "2", "--dry-launch", "--full", "--dump-outputs", str(tmp_path / "o")])
    assert d["dry_launch"] and d["world_size"] == 2
    assert not (tmp_path / "o").exists()               # nothing ran, nothing written


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_what_it_printed(tmp_path):
    out = str(tmp_path / "o")
    d = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(ROWS), "--dump-outputs", out])
    for k in HEADLINE_KEYS:
        assert k in d, k
    assert (d["steps"], d["warmup"], d["higher_is_better"], d["dtype"]) == (3, 1, True, "u64")
    assert d["unit"] == "joined tuples/s" and d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: rows of the result per second of a step
    # (ms_per_step is printed to 1e-3 ms, value to 0.1: half a unit of each is the whole difference)
    rows = d["config"]["result_rows"]
    assert rows > 0
    assert d["value"] == pytest.approx(rows / (d["ms_per_step"] * 1e-3), rel=0.0006 / d["ms_per_step"] + 1e-6)
    for k in FULL_ONLY_KEYS + ("cpu_baseline",):
        assert not d.get(k), k                         # nothing measured beside the timed steps
    stdout = d["config"]["stdout"]
    raw = np.load(os.path.join(out, "stdout_bytes.npy"))
    assert bytes(raw.astype(np.uint8)).decode() == stdout
    assert _u64(out) == [None if t == "NULL" else int(t) for t in stdout.split()]
    assert np.load(os.path.join(out, "result_rows.npy")).tolist() == [float(rows)]


@pytest.mark.gpu
def test_full_run_still_measures_everything_beside_the_line():
    d = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", str(ROWS), "--cpu-rows", str(ROWS),
                "--full"])
    for k in HEADLINE_KEYS + FULL_ONLY_KEYS:
        assert d.get(k), k
    assert d["parity"] is True and d["parity_detail"]["equals_faithful_executor"] is True
    for k in ("faithful_executor", "materialised_last_join", "two_stream_sorts"):
        assert d[k]["stdout_identical"] is True, k
    assert d["cpu_baseline"]["parity_with_gpu"] is True
    assert d["roofline"]["kernel"] in d["stages"]
