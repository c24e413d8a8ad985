"""bench.py's command line: the plain run's result line, --full's extra legs
and --dump-outputs (what the timed path computed, comparable run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    # bench.py adjusts OMP_NUM_THREADS at import; monkeypatch puts it back
    monkeypatch.setenv("OMP_NUM_THREADS", os.environ.get("OMP_NUM_THREADS", "2"))
    monkeypatch.syspath_prepend(REPO)
    import bench as mod
    return mod


def sample_index(bench, n):
    return np.sort(np.random.default_rng(bench.DUMP_SEED).integers(
        0, n, bench.DUMP_MAX_ELEMS, dtype=np.int64))


def test_dump_outputs_whole_when_small_sampled_when_large(bench, tmp_path):
    import torch
    n_big = bench.DUMP_MAX_ELEMS + 12345
    big = torch.arange(n_big, dtype=torch.float64)
    small = torch.tensor([1.5, float("nan"), -2.0, float("inf"), float("-inf")],
                         dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    assert sorted(os.listdir(tmp_path / "a")) == [
        "big.npy", "big_nonfinite.npy", "small.npy", "small_nonfinite.npy"]
    a_big = np.load(tmp_path / "a" / "big.npy")
    a_small = np.load(tmp_path / "a" / "small.npy")
    c_small = np.load(tmp_path / "a" / "small_nonfinite.npy")
    assert a_big.dtype == np.float64 and a_small.dtype == np.float64
    assert c_small.dtype == np.float32
    # every dumped array is finite; the codes say what the zeros stand for
    np.testing.assert_array_equal(a_small, [1.5, 0.0, -2.0, 0.0, 0.0])
    np.testing.assert_array_equal(c_small, [0, 1, 0, 2, 3])
    assert not np.load(tmp_path / "a" / "big_nonfinite.npy").any()
    # arange: the sampled values are the sample indices themselves
    np.testing.assert_array_equal(a_big, sample_index(bench, n_big).astype(np.float64))
    np.testing.assert_array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    # three arrays at the cap (f64 values + f32 codes) stay under the 64 MB
    # a dump may take
    assert 3 * bench.DUMP_MAX_ELEMS * (8 + 4) <= 64 * 1000 * 1000


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "smoke", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump_match_engine(bench, fdb, tmp_path):
    line = run_bench("--dump-outputs", str(tmp_path / "dump"))
    w = bench.WORKLOADS["smoke"]
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    samples = w["n_series"] * w["n_samples"]
    assert line["value"] == pytest.approx(samples / (line["ms_per_step"] / 1e3),
                                          rel=1e-9)
    # the extra legs stay out of a plain run
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["kernel_ms_per_step"] is None

    # the dump is what a caller of the timed path receives for the same inputs
    st = bench.build_store(w, rank=0)
    q = bench.make_query(w)
    eng = fdb.Engine(0)
    want = np.empty(st.num_series * q.num_windows, dtype=np.float64)
    eng.query(eng.upload(st), q, out=want)
    assert sorted(os.listdir(tmp_path / "dump")) == ["out.npy", "out_nonfinite.npy"]
    got = np.load(tmp_path / "dump" / "out.npy")
    code = np.load(tmp_path / "dump" / "out_nonfinite.npy")
    assert got.dtype == np.float64 and np.isfinite(got).all()
    assert want.size > bench.DUMP_MAX_ELEMS
    want = want[sample_index(bench, want.size)]
    # rate() leaves only NaN (a window with under two samples) as non-finite
    np.testing.assert_array_equal(code, np.isnan(want).astype(np.float32))
    np.testing.assert_array_equal(got, np.nan_to_num(want, nan=0.0, posinf=0.0,
                                                     neginf=0.0))
    assert 0 < code.sum() < got.size // 2


@pytest.mark.gpu
def test_full_run_adds_roofline_and_cpu_baseline():
    line = run_bench("--full")
    assert line["ms_per_step"] > 0 and line["kernel_ms_per_step"] > 0
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["achieved"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["kind"] == "port"
