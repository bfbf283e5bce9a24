"""bench.py's plain run and --dump-outputs.

A plain run (no --full) times the headline workload's steps and prints the
line; every leg that takes runs or checks of its own is behind --full.
--dump-outputs DIR writes what the last timed step left with its caller as
float .npy files (bench.dump_outputs).  On the CPU: dump_outputs on canned
verdicts (whole burst and seeded sample), the line of a plain run's result,
and the launcher's default deadline with and without --full.  On the GPU: one
plain run of the 100K-frame workload with --dump-outputs, its line and its
files against the oracle."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_bind as O
import rxdist
import rxgpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def cfg1_oracle():
    """the oracle's verdicts of the 100K-frame burst, as n x 16 bytes"""
    w = rxdist.WORKLOADS["cfg1"]
    cfg = rxdist.gen_cfg("cfg1")
    pk, off, ln = R.gen_host(cfg, 0, w["n"], w["unit_log2"])
    udp, tcb = R.gen_flows(cfg)
    v = O.Tables(udp, tcb).classify(pk, off, ln, w["unit_log2"])
    v = np.frombuffer(v.tobytes(), np.uint8).reshape(w["n"], 16).copy()
    v.setflags(write=False)
    return v, len(udp) + len(tcb)


def _load(d):
    got = {f: np.load(os.path.join(d, f + ".npy")) for f in ("verdicts", "verdict_frames",
                                                            "counts")}
    assert sorted(os.listdir(d)) == ["counts.npy", "verdict_frames.npy", "verdicts.npy"]
    assert got["verdicts"].dtype == np.float32
    assert got["verdict_frames"].dtype == np.float64 and got["counts"].dtype == np.float64
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    return got["verdicts"], got["verdict_frames"], got["counts"]


def test_dump_whole_burst(bench, cfg1_oracle, tmp_path):
    v, nflows = cfg1_oracle
    n = 1000  # fewer than DUMP_FRAMES: every frame; the buffer is longer than the burst
    out = torch.from_numpy(np.concatenate([v[:n].reshape(-1), np.full(64, 255, np.uint8)]))
    counts = torch.arange(7, dtype=torch.int64) * (1 << 40)
    bench.dump_outputs(str(tmp_path / "a" / "b"), out, n, counts)
    rows, frames, cnt = _load(str(tmp_path / "a" / "b"))
    assert rows.shape == (n, 16) and np.array_equal(rows, v[:n].astype(np.float32))
    assert np.array_equal(frames, np.arange(n, dtype=np.float64))
    assert np.array_equal(cnt, np.arange(7, dtype=np.float64) * 2.0 ** 40)


def test_dump_seeded_sample(bench, cfg1_oracle, tmp_path, monkeypatch):
    v, _ = cfg1_oracle
    n, m = len(v), 4096
    monkeypatch.setattr(bench, "DUMP_FRAMES", m)
    out = torch.from_numpy(v.reshape(-1).copy())
    counts = torch.zeros(1, dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "x"), out, n, counts)
    bench.dump_outputs(str(tmp_path / "y"), out, n, counts)
    rows, frames, _ = _load(str(tmp_path / "x"))
    rows2, frames2, _ = _load(str(tmp_path / "y"))
    assert np.array_equal(frames, frames2) and np.array_equal(rows, rows2)  # the same sample
    idx = frames.astype(np.int64)
    assert rows.shape == (m, 16) and len(np.unique(idx)) == m
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert idx[-1] - idx[0] > n // 2  # spread over the burst, not its head
    assert np.array_equal(rows, v[idx].astype(np.float32))


def test_plain_result_builds_the_line(bench):
    """a plain run's result (what run_workload returns without full) through
    build_line / compact_line: the headline fields, nulls for the legs"""
    w = rxdist.WORKLOADS["cfg2"]
    head = dict(workload="cfg2", desc=w["desc"], frames_per_step=w["n"], frames_this_rank=w["n"],
                nflows=1024, mpps=70000.0, gbps=6000.0, ms_per_step=0.2397, kernel_ms_avg=0.2391,
                rc0_frac=None, counts_ok=None, counts_match=None, parity=None, digest=None,
                roofline=dict(bound="hbm", achieved=6030.1, peak=8000.0, unit="GB/s", frac=0.7538,
                              traffic=None, kernel=None))
    line = bench.build_line(["cfg2"], {"cfg2": head}, 20, 5, 200.0, 1, 1, None)
    short = json.loads(json.dumps(bench.compact_line(line), separators=(",", ":")))
    assert short["value"] == 70000.0 and short["unit"] == "Mpps" and short["dtype"] == "u8"
    assert short["higher_is_better"] is True and short["ms_per_step"] == 0.2397
    assert short["steps"] == 20 and short["warmup"] == 5 and "metric" in short
    assert short["roofline"]["frac"] == 0.7538 and "kernel" not in short["roofline"]
    assert short["parity"] == dict(checked=None, mismatches=None)
    assert short["digest_ok"] is None and short["cpu_baseline"] is None
    assert not [k for k in short if k.startswith("cfg")] and "socket_api" not in short


def test_default_deadline_follows_full(bench):
    assert bench._deadline_arg(["--gpus", "2"]) == 120.0 + 120.0
    assert bench._deadline_arg(["--gpus", "2", "--full"]) == 120.0 + 4 * 120.0
    assert bench._deadline_arg(["--full", "--workload", "cfg2,cfg4"]) == 120.0 + 2 * 120.0
    assert bench._deadline_arg(["--full", "--deadline", "15"]) == 15.0


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(gpu_device, cfg1_oracle, tmp_path):
    """one plain run (the 100K-frame workload, 3 timed steps after 2 warmup
    steps): the line has the headline fields and none of the --full legs, no
    detail file is written, and the dumped verdicts and counts are the
    oracle's for every frame"""
    v, nflows = cfg1_oracle
    d = tmp_path / "dump"
    env = {k: x for k, x in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_DETAIL")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--workload", "cfg1", "--ramp-ms", "0", "--dump-outputs", str(d)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "Mpps" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value is the burst's frames over the step time, in Mpps, up to the
    # line's rounding: ms_per_step to 1e-4 ms, value to 0.01 Mpps
    ms, val = line["ms_per_step"], line["value"]
    assert ms >= 0.001 and val > 0
    assert val == pytest.approx(len(v) / ms / 1e3, rel=0.5e-4 / (ms - 0.5e-4) + 0.005 / val + 1e-9)
    assert line["parity"] == dict(checked=None, mismatches=None) and line["digest_ok"] is None
    assert line["cpu_baseline"] is None and line["hbm_read_ceiling_gbs"] is None
    assert line["detail"] is None and "socket_api" not in line and "verdict8" not in line
    assert "stage cfg1: timed steps" in r.stderr and "stage cfg1: parity" not in r.stderr
    rows, frames, cnt = _load(str(d))
    assert np.array_equal(frames, np.arange(len(v), dtype=np.float64))
    assert np.array_equal(rows, v.astype(np.float32))
    # one flow, every frame delivered: counted once per warmup and timed step
    assert len(cnt) == nflows and cnt[0] == 5.0 * len(v) and cnt.sum() == cnt[0]
