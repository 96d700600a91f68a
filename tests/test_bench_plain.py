"""bench.py's plain run and --dump-outputs (CPU, no GPU): a plain run's line
carries the headline figure only (what --full adds is refused or absent),
the timed window's roofline is the window's bytes over its time, and the
dump writes one float64 array per output with unwritten list entries masked."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import copgpu as cg  # noqa: E402


class FakeBuffer:
    """download() of a DeviceBuffer over host bytes."""

    def __init__(self, a):
        self.raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)

    def download(self, dtype, count, offset=0):
        n = np.dtype(dtype).itemsize * count
        return self.raw[offset:offset + n].copy().view(dtype)


@pytest.mark.parametrize("seg", [True, False])
def test_dump_outputs_writes_the_slot_as_float64(tmp_path, seg):
    B, P, slot = 600, 3, 2          # 600 packets: the last 256-packet segment is partial
    rng = np.random.default_rng(7)
    rec = np.zeros(P * B, cg.RESULT_DT)
    rec["verdict"] = rng.integers(0, 3, P * B)
    rec["flags"] = rng.integers(0, 4, P * B)
    rec["port"] = rng.integers(0, 65536, P * B)
    rec["route_nh"] = rng.integers(0, 2**32, P * B, dtype=np.uint64)
    per = (B + cg.SEG_PKTS - 1) // cg.SEG_PKTS if seg else 1
    width = cg.SEG_PKTS if seg else B
    cnt = rng.integers(0, min(width, B - (per - 1) * width) + 1, P * per).astype(np.uint32)
    fwd = rng.integers(0, 2**32, P * B, dtype=np.uint64).astype(np.uint32)   # stale words everywhere
    d = str(tmp_path / "out")
    bench.dump_outputs(d, slot, B, FakeBuffer(rec), FakeBuffer(fwd), FakeBuffer(cnt), seg)
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["flags", "fwd_count", "fwd_idx", "port", "route_nh", "verdict"]
    assert all(a.dtype == np.float64 for a in got.values())
    mine = rec[slot * B:(slot + 1) * B]
    for f in mine.dtype.names:
        assert np.array_equal(got[f], mine[f].astype(np.float64)), f
    c = cnt[slot * per:(slot + 1) * per]
    assert np.array_equal(got["fwd_count"], c.astype(np.float64))
    want = np.full(B, -1.0)
    for k in range(per):
        lo = k * width
        want[lo:lo + c[k]] = fwd[slot * B + lo:slot * B + lo + c[k]]
    assert np.array_equal(got["fwd_idx"], want)


def test_dump_outputs_without_lists(tmp_path):
    rec = np.zeros(8, cg.RESULT_DT)
    rec["port"] = np.arange(8)
    bench.dump_outputs(str(tmp_path), 1, 4, FakeBuffer(rec), None, None, True)
    assert sorted(os.listdir(tmp_path)) == ["flags.npy", "port.npy", "route_nh.npy", "verdict.npy"]
    assert np.array_equal(np.load(tmp_path / "port.npy"), [4.0, 5.0, 6.0, 7.0])


def test_timed_roofline_is_the_window():
    res = {"engine": "pmd", "bytes_per_pkt": 74.75, "total_pkts": 2 * 20 * 65536, "elapsed": 24.3e-6}
    r = bench.timed_roofline(res, 2)
    want = 74.75 * 20 * 65536 / 24.3e-6 / 1e9
    assert r["achieved"] == pytest.approx(want, rel=1e-3)
    assert r["frac_timed"] == pytest.approx(want / bench.HBM_PEAK_GBS, abs=1e-4)
    assert bench.timed_roofline({"engine": "pmd"}, 1) is None      # no packets counted


def run(*args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=120, env=env)


def test_plain_dry_run_has_the_headline_only():
    r = run("--gpus", "1", "--dry-run", "--steps", "4", "--warmup", "1", "--repeats", "1")
    assert r.returncode == 0, r.stderr
    j = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    assert j["steps"] == 4 and j["value"] > 0
    assert "secondary" not in j and "cpu_baseline" not in j


def test_secondary_needs_full():
    r = run("--gpus", "1", "--dry-run", "--secondary", "fw_lpm")
    assert r.returncode != 0 and "--full" in r.stderr
