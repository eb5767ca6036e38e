"""The row filter's plan compiler under AddressSanitizer + UBSan on the CPU: tests/hostcheck/filter_plan_check.cpp compiles
orc_rust_amd/csrc/orcgpu_filter_plan.inc -- the text liborcgpu.so is built from -- into a stand-alone program and feeds it
well-formed and malformed node lists.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_plan") / "filter_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_plan_check.cpp")])
    out = subprocess.run([exe, "5", "3000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def test_well_formed_lists_compile(lines):
    got = {ln[0]: (int(ln[1]), int(ln[2]), int(ln[3])) for ln in lines if ln[0] != "random"}
    assert got["leaf"] == (OK, 1, 1)
    assert got["and3"] == (OK, 5, 2)          # three leaves, two binary ANDs
    assert got["empty_and"] == (OK, 1, 1) and got["empty_or"] == (OK, 1, 1)
    assert got["null_literal"] == (OK, 1, 1)
    assert got["depth_at_limit"][0] == OK and got["depth_at_limit"][2] == 64
    assert got["right_deep_at_limit"][0] == OK


def test_malformed_lists_are_refused_with_their_codes(lines):
    got = {ln[0]: int(ln[1]) for ln in lines if ln[0] != "random"}
    for name in ("children_past_end", "children_4_billion", "not_without_child", "left_over", "unknown_op", "negative_op", "null_column",
                 "null_column_null_test", "unknown_column", "no_columns", "string_len_no_bytes", "no_nodes", "depth_over_limit",
                 "right_deep_over_limit"):
        assert got[name] == INVALID, name
    assert got["type_pair"] == MISMATCHED and got["bad_value_type"] == MISMATCHED
    assert got["timestamp_compare"] == UNSUPPORTED


def test_random_lists_return(lines):
    last = [ln for ln in lines if ln[0] == "random"][0]
    assert int(last[1]) == 3000 and 0 < int(last[2]) < 3000
