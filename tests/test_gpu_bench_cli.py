"""bench.py's command line on the GPU: a plain run measures the headline
figure alone (no CPU baseline, no stream floor, no PMC lookup: null in the
line), --full adds them, --steps is the number of timed steps, and
--dump-outputs writes what the last timed step computed -- the hit counters
and a fixed sample of the verdicts, float64 / float32 -- equal to the
oracle's over the same stream.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N = 1 << 18


def _bench(*extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--settle-ms", "20", "--packets", str(N)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def test_plain_run_dumps_its_outputs(tmp_path):
    import oracle
    from vpp_amd import workload
    d = tmp_path / "out"
    k = 1 << 14
    line = _bench("--dump-outputs", str(d), "--dump-sample", str(k))
    assert line["full"] is False and line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None
    assert line["roofline"]["stream_floor_ms"] is None and line["roofline"]["traffic"] is None
    assert line["roofline"]["kernel_ms_avg"] > 0 and line["counters_sum_ok"] is True
    assert sorted(os.listdir(d)) == ["counters.npy", "verdict_index.npy", "verdicts.npy"]
    counters, idx, verdicts = (np.load(d / f) for f in ("counters.npy", "verdict_index.npy", "verdicts.npy"))
    assert counters.dtype == np.float64 and idx.dtype == np.float64 and verdicts.dtype == np.float32
    acl, spec, _ = workload.config(3)
    tr = oracle.gen_traffic_v4(spec, 0, N)
    ov, oc = oracle.classify_fast(oracle.rules_to_c(acl.rules), tr["src"], tr["dst"], tr["dport"], tr["proto"])
    np.testing.assert_array_equal(counters, oc.astype(np.float64))
    ii = idx.astype(np.int64)
    assert len(ii) == k and np.all(np.diff(ii) >= 0) and ii[0] >= 0 and ii[-1] < N
    assert len(np.unique(ii)) > k // 2                 # a sample over the batch, not a prefix or one packet
    np.testing.assert_array_equal(verdicts, ov[ii].astype(np.float32))
    # the same packets on every run: the sample is seeded, not drawn afresh
    np.testing.assert_array_equal(ii, np.sort(np.random.default_rng(0xC0175EED).integers(0, N, k)))


def test_batch_within_the_sample_is_dumped_whole(tmp_path):
    d = tmp_path / "out"
    _bench("--dump-outputs", str(d))
    np.testing.assert_array_equal(np.load(d / "verdict_index.npy"), np.arange(N, dtype=np.float64))
    assert np.load(d / "verdicts.npy").shape == (N,)


def test_full_run_adds_the_baselines():
    line = _bench("--full", "--cpu-sample", "4096", "--faithful-sample", "64")
    assert line["full"] is True and line["ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["faithful"]["value"] > 0
    r = line["roofline"]
    assert r["stream_floor_ms"] > 0 and len(r["stream_floor_shapes_ms"]) >= 1
    assert r["traffic_source"] != "not read (--full)"
