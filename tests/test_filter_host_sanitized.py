"""The row filter call's host arithmetic under AddressSanitizer + UBSan on the CPU: tests/hostcheck/filter_host_check.cpp compiles
orc_rust_amd/csrc/orcgpu_filter_host.inc -- the text liborcgpu.so is built from -- into a stand-alone program that compares
filter_col_kind, filter_check_kinds, FilterWorkspace and filter_place_output with transcriptions of the code result_filter_plan
held before, over a seeded sweep of small shapes.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OFFSET_OVERFLOW = 5


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_host") / "filter_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_host_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    return [ln.split() for ln in out.stdout.splitlines()]


def test_every_shape_agrees_with_the_transcriptions(lines):
    assert not [ln for ln in lines if "MISMATCH" in ln]
    assert [ln for ln in lines if ln[0] == "kinds"] == [["kinds", "0"]]
    sweep = [ln for ln in lines if ln[0] == "sweep"]
    # B in {1, 64, 100, 8192} x six kept row counts x 0 .. 5 columns x n_segs in {0, 1, 3} x null counts zero / non-zero
    assert sweep == [["sweep", str(4 * 6 * 6 * 3 * 2), "0"]]
    assert lines[-1] == ["bad", "0"]


def test_a_batch_of_2_to_the_31_string_bytes_is_an_offset_overflow(lines):
    over = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "overflow"]
    # (status, batch, column): the lowest failing batch wins; at 2^31 - 1 bytes a batch is still fine
    assert over == [[OFFSET_OVERFLOW, 1, 2], [OFFSET_OVERFLOW, 2, 1], [0, 0, 0]]
