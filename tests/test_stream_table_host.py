"""csrc/stream_table.h -- the table of (device, stream) blocks behind every scratch block of the update kernels -- checked on the
host: tests/stream_table_check.cpp is compiled against the header with the host C++ compiler (the header makes no HIP call and
includes no HIP header) and run; every property it checks prints one "ok ..." line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe-policy-optimization_amd", "csrc")
PROPERTIES = [
    "find after add",
    "distinct keys give distinct blocks",
    "add succeeds CAP times",
    "add fails at CAP",
    "a refused add leaves the table as it was",
    "release by stream returns the stream's block count",
    "release by stream removes exactly that stream's blocks on that device",
    "the callback runs once per removed block",
    "swap-remove leaves the survivors findable",
    "releasing a stream without blocks returns 0",
    "a null stream without all releases nothing",
    "a released key can be added again",
    "release with all empties that device only",
    "the callback runs once per block of the device",
    "release with all ignores the stream argument",
    "an emptied table takes CAP blocks again",
]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("stream_table") / "stream_table_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                            os.path.join(ROOT, "tests", "stream_table_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    return run.returncode, run.stdout.splitlines()


def test_program_ends_clean(output):
    rc, lines = output
    assert rc == 0 and lines[-1] == "done 0", lines
    assert not [l for l in lines if l.startswith("FAIL")]


@pytest.mark.parametrize("prop", PROPERTIES)
def test_property(output, prop):
    _, lines = output
    assert f"ok {prop}" in lines, [l for l in lines if prop in l]
