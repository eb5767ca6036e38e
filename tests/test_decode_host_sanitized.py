"""The decode call's host planning under AddressSanitizer + UBSan on the CPU: tests/hostcheck/decode_host_check.cpp compiles
orc_rust_amd/csrc/orcgpu_decode_host.inc -- the text liborcgpu.so is built from -- into a stand-alone program.  The job layout
(layout_jobs) and the dealing of root columns to lanes (deal_lanes) must equal field by field what the code blocks gave that
decode_lane and decode_staged_once held before (kept in the program), over seeded random calls and the edge cases written out by
hand there.  The gathering of the roots' weights from the staged stripes (choose_lanes in orcgpu_decode.inc) needs the staged
types and is not part of the program: it is covered by the GPU parity tests only (tests/test_gpu_zstd_lanes.py,
tests/test_gpu_decode_crossing.py under ORCGPU_LANES).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g1", "-O0"]
CASES = ["layout, random", "layout, no jobs", "layout, one empty stream", "layout, a class without a job between two used ones",
         "layout, only the deepest PRESENT class", "layout, byte RLE of 511, 512, 1023 and 1024 blocks", "layout, no expected values",
         "layout, a call of 64 x kGroupTarget blocks and one block less", "layout, 2^32 blocks and one tile less",
         "lanes, random", "lanes, one root", "lanes, more lanes wanted than roots", "lanes, the first root a quarter of the call, and one byte less",
         "lanes, longest block of 4095 and of 4096 sequences", "lanes, two lanes with one sequence less than the table scale and at it",
         "lanes, every root heavy", "lanes, four forced of which the last two stay empty", "lanes, equal weights"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decode_host") / "decode_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "decode_host_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout.splitlines()


def test_layout_and_lanes_equal_the_blocks_they_were_taken_from(lines):
    assert lines[-1] == "checked %d cases, 0 mismatches" % len(CASES), lines[-3:]
    assert [ln.rsplit(": ", 2)[0] for ln in lines[:-1]] == CASES
    assert all(ln.endswith(": same") for ln in lines[:-1]), [ln for ln in lines if not ln.endswith(": same")]


def test_random_cases_are_thousands(lines):
    sizes = {ln.rsplit(": ", 2)[0]: ln.rsplit(": ", 2)[1] for ln in lines[:-1]}
    assert sizes["layout, random"] == "3000 calls" and sizes["lanes, random"] == "4000 calls"
