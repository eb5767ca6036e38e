"""The conditions of an aggregate list -- agg(x) FILTER (WHERE ...) -- through the plan compilers under AddressSanitizer + UBSan on
the CPU: tests/hostcheck/agg_filter_plan_check.cpp compiles orc_rust_amd/csrc/orcgpu_agg_plan.inc and orcgpu_filter_plan.inc -- the
text liborcgpu.so is built from -- into a stand-alone program that builds its own cases and prints one line per fact.  Sharing by
node-wise equality, the limit of 64 distinct conditions, the row filter's refusals with its statuses and messages, the bounds check
in front of every launch, and where programs, planes and literals lie in a list that mixes LIKE, IN and comparisons, alone and
behind a row filter.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
FOP_CMP_FLOAT, FOP_CMP_STRING, FOP_AND, FOP_LIKE, FOP_IN = 1, 3, 10, 13, 14
LIKE_PREFIX, LIKE_GENERAL, IN_KEY_I64 = 1, 4, 0


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("agg_filter_plan") / "agg_filter_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "agg_filter_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[f[0]] = (f[1:], msg)
    return got


def ints(out, name):
    return [int(x) for x in out[name][0]]


def test_identical_conditions_share_a_plane_and_different_ones_do_not(out):
    # rc, distinct conditions, then the cond of every instruction: A, A again from other pointers, B, none, C
    assert ints(out, "share") == [OK, 3, 1, 1, 2, 0, 3]
    assert ints(out, "share_program") == [3, 0, 1, 2, 1]            # three one-leaf programs, one behind the other
    # 'abc', 'abd', 'abc' again, the NULL literal, < 0.0 and < -0.0 (other bits): only the repeated one is shared
    assert ints(out, "bytes") == [OK, 5, 1, 2, 1, 3, 4, 5]
    assert ints(out, "null_filters") == [OK, 0, 0]


def test_avg_carries_its_condition_and_the_kept_rows_instruction_has_none(out):
    assert ints(out, "avg") == [OK, 1, 1, 1]                        # (AVG is one instruction: its sum, finished over the count of values)
    assert ints(out, "kept_rows") == [0, 32]                        # cond = 0, and the instruction is still 32 bytes


def test_64_distinct_conditions_are_accepted_and_65_refused(out):
    assert ints(out, "conds_64") == [OK, 64, 1, 64]
    assert ints(out, "conds_65") == [INVALID] and "64" in out["conds_65"][1] and "distinct conditions" in out["conds_65"][1]
    assert ints(out, "specs_64") == [OK, 1]
    assert ints(out, "specs_65") == [INVALID] and "aggregates" in out["specs_65"][1]


def test_the_row_filters_refusals_with_its_statuses_and_messages(out):
    for name, code, words in (("unknown_column", INVALID, ("row filter:", "'nope'", "not a projected root column")),
                              ("too_deep", INVALID, ("row filter:", "deeper than 64")),
                              ("dict_column", UNSUPPORTED, ("row filter:", "'dict'", "dictionary column")),
                              ("literal_kind", MISMATCHED, ("row filter:", "'i64'")),
                              ("nodes_left", INVALID, ("row filter:", "left behind")),
                              ("count_without_nodes", INVALID, ("aggregate 0",))):
        assert ints(out, name) == [code], name
        for w in words:
            assert w in out[name][1], (name, out[name][1])
    assert ints(out, "deep_64") == [OK, 64]
    assert ints(out, "dict_null_test") == [OK]


def test_the_bounds_check_refuses_a_cond_past_the_planes(out):
    # both conds among two planes; among one; a cond of 3 among two; no cond and no plane
    assert ints(out, "bounds") == [1, 0, 0, 1]
    # the spans inside the program; shifted past its end; shifted inside a longer one
    assert ints(out, "span_bounds") == [1, 0, 1]


def test_offsets_of_a_list_mixing_like_in_and_comparisons(out):
    # LIKE, IN, a float comparison, a string EQ, AND(LIKE, IN with a NULL), and the first LIKE again
    assert ints(out, "mixed") == [OK, 5, 1, 2, 3, 4, 5, 1]
    assert out["mixed_spans"][0] == ["0+1", "1+1", "2+1", "3+1", "4+3"]
    assert ints(out, "mixed_ops") == [FOP_LIKE, FOP_IN, FOP_CMP_FLOAT, FOP_CMP_STRING, FOP_LIKE, FOP_IN, FOP_AND]
    assert ints(out, "mixed_planes") == [4, 0, 1, 2, 3]             # numbered together, in leaf order
    assert out["mixed_leaves"][0] == ["like", "0", "4", "in", "1", "5"]
    assert ints(out, "mixed_sound") == [1]
    shape1, eq_bytes, shape2, in_kind, in2_keys, in2_null = out["mixed_lits"][0]
    assert (int(shape1), eq_bytes, int(shape2), int(in_kind), int(in2_keys), int(in2_null)) == (LIKE_PREFIX, "abc", LIKE_GENERAL, IN_KEY_I64, 2, 1)
    # behind a row filter OR(LIKE, IN): three instructions and two planes in front, nothing of either changed
    rc, first, planes, same_front, same_back, sound, *cond_planes = ints(out, "behind_row_filter")
    assert (rc, first, planes, same_front, same_back, sound) == (OK, 3, 6, 1, 1, 1)
    assert cond_planes == [2, 3, 4, 5]
    assert out["behind_leaves"][0] == ["like", "0", "3", "7", "in", "1", "4", "8"]
