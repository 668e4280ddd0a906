"""The entry writer of zk-proof-of-assets_amd/csrc/host_files.hpp (put_text, put_entries with its round hook, write_entries)
on the CPU: tools/entry_writer_check.cpp includes the header's own text, g++ compiles it without HIP, and a run writes N
entries three ways and reads them back. Sizes: nothing, a few, exactly one round of 2^16, and two rounds and a bit.
ENTRY_WRITER_CHECK_FLAGS adds compiler flags (a sanitizer build of this stand-alone program)."""
import os
import shlex
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("entry_writer") / "entry_writer_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread"] + shlex.split(os.environ.get("ENTRY_WRITER_CHECK_FLAGS", "")) +
                   ["-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"),
                    os.path.join(ROOT, "tools", "entry_writer_check.cpp"), "-o", out], check=True, capture_output=True, text=True)
    return out


@pytest.mark.parametrize("threads", ["1", "5"])
@pytest.mark.parametrize("n,rounds", [(0, 0), (7, 1), (1 << 16, 1), ((1 << 17) + 9, 3)])
def test_entry_writer_round_trip(check_bin, tmp_path, n, rounds, threads):
    rc = subprocess.run([check_bin, str(tmp_path), str(n)], capture_output=True, text=True, timeout=300,
                        env=dict(os.environ, ZKPOA_SETUP_THREADS=threads))
    assert (rc.returncode, rc.stdout, rc.stderr) == (0, "ok %d entries, %d rounds\n" % (n, rounds), "")
    assert sorted(os.listdir(tmp_path)) == ["a.json", "b.json"]                        # no temporary file, no c.json
