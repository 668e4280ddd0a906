"""zk-proof-of-assets_amd/csrc/host_threads.hpp on the CPU: tools/host_threads_check.cpp includes the header's own text, g++
compiles it without HIP (with the spawn seam that only this program sees), and each case is a sub-command that prints one
line and exits 0. A run that ends on a signal has a negative status and fails. HOST_THREADS_CHECK_FLAGS adds compiler flags
(a sanitizer build)."""
import os
import shlex
import subprocess

import pytest

from conftest import ROOT

MIN_PER_THREAD = 1000
THREADS = 4


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_threads") / "host_threads_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-DHOST_THREADS_CHECK_SPAWN_HOOK"] +
                   shlex.split(os.environ.get("HOST_THREADS_CHECK_FLAGS", "")) +
                   ["-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_threads_check.cpp"), "-o", out], check=True, capture_output=True, text=True)
    return out


def case(check_bin, *args, env=None):
    rc = subprocess.run([check_bin] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                        env=dict(os.environ, **(env or {})))
    assert rc.returncode == 0, (rc.returncode, rc.stdout, rc.stderr[-2000:])
    assert rc.stdout.endswith("\n") and rc.stdout.count("\n") == 1 and rc.stderr == "", (rc.stdout, rc.stderr[-2000:])
    return rc.stdout[:-1]


@pytest.mark.parametrize("threads", [1, 4, 32])
def test_run_threads_visits_every_index_once(check_bin, threads):
    assert case(check_bin, "visit", threads) == "visited %d: each index once" % threads


def test_first_error_by_index_after_all_have_joined(check_bin):
    assert case(check_bin, "first-error") == "caught 2 with 8 bodies finished"


@pytest.mark.parametrize("count,pieces", [(0, 1), (1, 1), (MIN_PER_THREAD - 1, 1), (MIN_PER_THREAD * THREADS + 1, THREADS)])
def test_parallel_ranges_cover_the_range(check_bin, count, pieces):
    got = case(check_bin, "ranges", count, MIN_PER_THREAD, env={"ZKPOA_SETUP_THREADS": str(THREADS)})
    assert got == "covered %d in %d ranges" % (count, pieces)


def test_side_task_get_rethrows_once(check_bin):
    assert case(check_bin, "get-once") == "boom once, then quiet"


def test_side_task_destructor_joins(check_bin):
    assert case(check_bin, "destructor") == "flag seen after the scope"


def test_side_task_move_assign_waits_for_the_old_task(check_bin):
    assert case(check_bin, "move-assign") == "old task done when the assignment returned"


def test_writer_owns_its_section_while_the_scope_unwinds(check_bin):
    """the shape of `zkey new`: 64 MiB of the bytes 0..255 in turn, summed by a writer let go after the throw"""
    assert case(check_bin, "zkey-new") == "sum %d" % ((64 << 20) // 256 * sum(range(256)))


@pytest.mark.parametrize("how", ["run", "tasks"])
def test_a_thread_that_cannot_be_started_is_an_error_not_the_end(check_bin, how):
    assert case(check_bin, "spawn-fail", how) == "system_error, 2 bodies ran"
