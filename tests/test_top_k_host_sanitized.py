"""The host side of ORDER BY ... LIMIT k under AddressSanitizer + UBSan on the CPU: tests/hostcheck/top_k_host_check.cpp compiles
orc_rust_amd/csrc/orcgpu_top_k_host.inc and device/top_k_program.h -- the text liborcgpu.so is built from -- into a stand-alone
program that builds its own cases and prints one line per fact.  The plan per key-kind list with its lengths and order, the pass
plan, the workspace offsets, the key-record comparison on the hand cases of tests/test_top_k_model.py (the expected orders are the
same lists), the k-way merge, and the refusals with their statuses and messages.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
TK_INT, TK_BOOL, TK_FLOAT, TK_DEC128 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_k_host") / "top_k_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "top_k_host_check.cpp")])
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


def keys_of(out, name):
    """rc, n, len, then per key (col, kind, descending, nulls_first, first, bytes)"""
    f = out[name][0]
    return int(f[0]), int(f[1]), int(f[2]), [tuple(int(x) for x in k.split(":")) for k in f[3:]]


def test_the_plan_per_key_kind_list_with_its_lengths_and_order(out):
    assert keys_of(out, "one_i64") == (OK, 1, 9, [(0, TK_INT, 0, 0, 0, 9)])
    assert keys_of(out, "desc_nf") == (OK, 1, 9, [(1, TK_FLOAT, 1, 1, 0, 9)])
    assert keys_of(out, "date") == (OK, 1, 9, [(9, TK_INT, 0, 0, 0, 9)])
    assert keys_of(out, "one_dec") == (OK, 1, 17, [(3, TK_DEC128, 0, 0, 0, 17)])
    # Decimal desc, Boolean, Timestamp(ns as int64) nulls first, Byte with flags that are any non-zero value: 17 + 9 + 9 + 9 bytes
    assert keys_of(out, "four_mixed") == (OK, 4, 44, [(3, TK_DEC128, 1, 0, 0, 17), (2, TK_BOOL, 0, 0, 17, 9), (6, TK_INT, 0, 1, 26, 9), (10, TK_INT, 1, 1, 35, 9)])
    assert keys_of(out, "k_max")[0] == OK


def test_the_pass_plan_is_the_key_strings_bytes_forwards_then_backwards(out):
    sel = ["0.%d" % b for b in range(9)] + ["1.%d" % b for b in range(17)]
    assert out["i64_dec_select"][0] == ["26"] + sel
    assert out["i64_dec_sort"][0] == ["26"] + sel[::-1]
    assert out["b_select"][0] == ["9"] + ["0.%d" % b for b in range(9)]
    assert out["b_sort"][0] == ["9"] + ["0.%d" % b for b in range(8, -1, -1)]


def test_the_refusals_with_their_statuses_and_messages(out):
    for name, code, words in (("no_key", INVALID, ("no sort key",)),
                              ("five_keys", INVALID, ("more than", "4")),
                              ("k_zero", INVALID, ("k must be", "65536")),
                              ("k_over", INVALID, ("k must be", "65536")),
                              ("unknown", INVALID, ("'nope'", "not a projected root column")),
                              ("twice", INVALID, ("'i64'", "listed twice")),
                              ("null_name", INVALID, ("without a column name",)),
                              ("string_key", UNSUPPORTED, ("'s'", "String")),
                              ("binary_key", UNSUPPORTED, ("'bin'", "Binary")),
                              ("dict_key", UNSUPPORTED, ("'dict'", "dictionary column")),
                              ("ts_dec_key", UNSUPPORTED, ("'ts_dec'", "Decimal128(38, 9)")),
                              ("nested", UNSUPPORTED, ("'st'", "nested"))):
        assert ints(out, name) == [code], name
        assert out[name][1].startswith("top-k:"), out[name][1]
        for w in words:
            assert w in out[name][1], (name, out[name][1])


def test_the_workspace_is_aligned_in_order_and_inside_its_bytes(out):
    # aligned, non-overlapping and ascending, the last piece inside `bytes`; then cap, record stride, select blocks, sort blocks, record bytes
    assert ints(out, "ws_small") == [1, 1, 1, 10, 16, 274, 1, 160]              # 70001 rows: 1094 words, 4 a block
    assert ints(out, "ws_k_above_rows") == [1, 1, 1, 63, 72, 1, 1, 63 * 72]     # cap = the rows; four Decimal keys: 68 -> 72
    assert ints(out, "ws_big") == [1, 1, 1, 65536, 32, 1024, 32, 65536 * 32]    # the select's grid is capped, the sort's is k / 2048
    assert ints(out, "ws_one_row") == [1, 1, 1, 1, 16, 1, 1, 16]
    assert ints(out, "stride") == [16, 24, 32, 72]


def test_key_records_compare_as_the_header_says(out):
    # (the lists of tests/test_top_k_model.py, same inputs)
    assert ints(out, "nan_inf_asc") == [2, 5, 3, 1, 0, 4]
    assert ints(out, "nan_inf_desc") == [0, 4, 1, 3, 5, 2]
    assert ints(out, "zeros_asc") == [4, 0, 1, 2, 3]
    assert ints(out, "zeros_desc") == [0, 1, 2, 3, 4]
    assert ints(out, "nulls_asc") == [2, 4, 0, 1, 3]
    assert ints(out, "nulls_desc") == [0, 4, 2, 1, 3]
    assert ints(out, "nulls_desc_first") == [1, 3, 0, 4, 2]
    assert ints(out, "nulls_asc_first") == [1, 3, 2, 4, 0]
    assert ints(out, "int64_asc") == [2, 3, 0, 4, 1]
    assert ints(out, "int64_desc") == [1, 4, 0, 3, 2]
    assert ints(out, "dec_asc") == [1, 3, 2, 0, 4]
    assert ints(out, "dec_desc_first") == [4, 0, 2, 3, 1]
    assert ints(out, "bools") == [1, 4, 0, 3, 2]
    assert ints(out, "four_keys_0") == [1, 4, 3, 0, 2]
    assert ints(out, "four_keys_1") == [2, 0, 3, 1, 4]


def test_the_merge_over_stripes_with_ties_an_empty_stripe_and_a_small_cap(out):
    # stripes [1 3 3 7] [] [0 3 8] [3 3] stand at 0, 4, 4, 7 of the hand-out: ties on 3 by stripe, then by position
    assert out["merge_all"][0] == ["0", "9", "4", "0", "1", "2", "5", "7", "8", "3", "6", "guard=777"]
    assert out["merge_k5"][0] == ["0", "5", "4", "0", "1", "2", "5", "guard=777"]
    assert out["merge_cap_small"][0] == [str(INVALID), "5", "guard=777"]        # *n is set, nothing written
    assert out["merge_cap_zero"][0] == [str(INVALID), "5", "guard=777"]
    assert out["merge_empty"][0] == ["0", "0", "guard=777"]
    assert out["merge_none"][0] == ["0", "0", "guard=777"]
