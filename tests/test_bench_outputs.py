"""bench.py's plain run and --dump-outputs: the line of a plain run holds the headline alone, --steps sets the number
of timed steps, and the dumped arrays are what the last timed step computed (here: the known-dlog expectation of the
seeded MSM, from the oracle's scalar multiplication)."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_field_rows_are_exact_and_the_dump_is_bounded(tmp_path):
    import bench
    vals = [0, 1, bench.R_MOD - 1, (1 << 256) - 1, 0x1234_5678_9ABC_DEF0 << 130]
    rows = bench.field_rows(b"".join(v.to_bytes(32, "little") for v in vals))
    assert rows.dtype == np.float64 and rows.shape == (len(vals), 16)
    assert [sum(int(x) << (16 * i) for i, x in enumerate(r)) for r in rows] == vals
    bench.write_outputs(str(tmp_path / "d"), {"a": rows})
    assert np.array_equal(np.load(tmp_path / "d" / "a.npy"), rows)
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not (tmp_path / "e").exists()


def test_bench_help_names_the_plain_and_full_options():
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                        timeout=60, cwd=ROOT)
    assert rc.returncode == 0 and "--full" in rc.stdout and "--dump-outputs" in rc.stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_result(zk, tmp_path):
    import bench
    from zkpoa_amd.synthetic import dlog_sums
    logn, steps = 14, 3
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "msm_g1_2p%d" % logn,
                         "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert rc.returncode == 0, rc.stderr[-2000:]
    line = json.loads([l for l in rc.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "pts/s"
    assert line["value"] == pytest.approx((1 << logn) * 1e3 / line["ms_per_step"])
    assert "also" not in line and "roofline" not in line and "cpu_baseline" not in line
    assert sorted(os.listdir(tmp_path / "out")) == ["msm_g1_point.npy"]
    # the inputs bench.py seeds: bases (a + i*b)*G, scalars from np_scalars -> the sum has discrete log a*s0 + b*s1
    seeds = random.Random(0x5EED0001)
    a, b = seeds.randrange(bench.R_MOD), seeds.randrange(bench.R_MOD)
    s0, s1 = dlog_sums(bench.np_scalars(1 << logn, 0x5EED0002), 0)
    want = bench.field_rows(bench.oracle_g1((a * s0 + b * s1) % bench.R_MOD))
    assert np.array_equal(np.load(tmp_path / "out" / "msm_g1_point.npy"), want)
