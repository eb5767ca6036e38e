"""The decompressors' table builder under AddressSanitizer + UBSan on the CPU: tests/hostcheck/decomp_plan_check.cpp compiles
orc_rust_amd/csrc/orcgpu_decomp_plan.inc -- the text liborcgpu.so is built from -- into a stand-alone program.  The tables a staged
stream carries, merged and rebased for a call, must equal field by field the tables built from the call's chunk lists directly
(the builder a decode call ran before the streams carried their tables, kept in the program).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g1", "-O0"]
CASES = ["one stripe", "three stripes, equal counts", "three stripes, equal counts, other order", "no compressed block in the middle stripe",
         "only a stripe without compressed blocks", "original chunk, nseq 0, raw / RLE literals, bad chunk, unknown size", "... between two stripes",
         "chunk lists that are subsets", "some streams of each stripe", "the same stream alone", "the same stream with another partner",
         "chunks above the top bucket", "snappy", "lz4", "zlib", "one stream of five"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decomp_plan") / "decomp_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "decomp_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout.splitlines()


def test_merged_tables_equal_the_tables_built_per_call(lines):
    assert lines[-1] == "checked %d calls, 0 mismatches" % len(CASES), lines[-3:]
    assert [ln.rsplit(": ", 2)[0] for ln in lines[:-1]] == CASES
    assert all(ln.endswith(": same") for ln in lines[:-1]), [ln for ln in lines if not ln.endswith(": same")]


def test_cases_have_blocks_to_order(lines):
    """the cases are not empty ones: the tie and merge cases hold dozens of blocks over several streams"""
    sizes = {ln.rsplit(": ", 2)[0]: [int(w) for w in ln.rsplit(": ", 2)[1].replace(",", "").split() if w.isdigit()] for ln in lines[:-1]}
    assert sizes["three stripes, equal counts"][0] == 11 and sizes["three stripes, equal counts"][2] >= 30
    assert sizes["only a stripe without compressed blocks"][2] == 0
    assert sizes["zlib"][1] == 8
