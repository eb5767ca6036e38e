"""The aggregation's plan compiler and record arithmetic under AddressSanitizer + UBSan on the CPU:
tests/hostcheck/agg_plan_check.cpp compiles orc_rust_amd/csrc/orcgpu_agg_plan.inc -- the text liborcgpu.so is built from -- into a
stand-alone program.  Every (op, column kind) pair of the table in include/orcgpu.h and its status, the scale rule of the Decimal
product, the limit of 64 specs, a missing column; and the 192-bit merge with its range checks against Python ints, over random
words and over the carries at 2^64 - 1, 2^127 - 1 and +-(10^38 - 1).  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
COUNT_ROWS, COUNT, SUM, MIN, MAX, SUM_PRODUCT = range(6)
AK_COUNT_ROWS, AK_COUNT, AK_SUM_INT, AK_SUM_DEC, AK_SUM_F64, AK_SP_INT, AK_SP_DEC, AK_SP_F64, AK_MINMAX_INT, AK_MINMAX_DEC, AK_MINMAX_F64 = range(11)
KIND_U64, KIND_I128, KIND_DEC128, KIND_F64, KIND_I64 = range(5)
CLASSES = {
    "int": ["i8", "i16", "i32", "i64", "i64_as_i16"], "date": ["date"], "bool": ["b"], "float": ["f32", "f64"],
    "dec": ["dec15_2", "dec38_0", "dec38_19"], "ts": ["ts", "ts_us", "tsi"], "ts9": ["ts9"], "str": ["s", "bin", "vc", "ch"], "dict": ["dict"],
}
SCALE = {"dec15_2": 2, "dec38_0": 0, "dec38_19": 19, "dec38_20": 20}
UNIT = {"ts": 3, "ts_us": 2, "tsi": 3}
# class -> what SUM, MIN / MAX and SUM_PRODUCT with itself become: an AK_* kind, or the refusal
SUM_OF = {"int": AK_SUM_INT, "float": AK_SUM_F64, "dec": AK_SUM_DEC, "date": -MISMATCHED, "bool": -MISMATCHED, "ts": -MISMATCHED, "str": -MISMATCHED,
          "dict": -UNSUPPORTED, "ts9": -UNSUPPORTED}
MINMAX_OF = {"int": AK_MINMAX_INT, "date": AK_MINMAX_INT, "bool": AK_MINMAX_INT, "ts": AK_MINMAX_INT, "float": AK_MINMAX_F64, "dec": AK_MINMAX_DEC,
             "str": -MISMATCHED, "dict": -UNSUPPORTED, "ts9": -UNSUPPORTED}
SP_OF = {"int": AK_SP_INT, "float": AK_SP_F64, "dec": AK_SP_DEC, "date": -MISMATCHED, "bool": -MISMATCHED, "ts": -MISMATCHED, "str": -MISMATCHED,
         "dict": -UNSUPPORTED, "ts9": -UNSUPPORTED}
M192 = (1 << 192) - 1
RNG = np.random.default_rng(23)


def words(v):
    v &= M192
    return ["%x" % ((v >> (64 * k)) & (2 ** 64 - 1)) for k in range(3)]


def signed(ws):
    v = sum(int(w, 16) << (64 * k) for k, w in enumerate(ws))
    return v - (1 << 192) if v >> 191 else v


def rand192(bits):
    v = int.from_bytes(RNG.bytes(24), "little") & ((1 << bits) - 1)
    return -v if RNG.random() < 0.5 else v


T38 = 10 ** 38
MERGES = {
    "carry_w0": (2 ** 64 - 1, 1), "carry_w1": (2 ** 128 - 1, 1), "carry_both": (2 ** 128 - 1, 2 ** 64 + 1), "borrow": (0, -1), "borrow_w1": (2 ** 64, -1),
    "borrow_w2": (2 ** 128, -1), "i128_max": (2 ** 127 - 2, 1), "i128_over": (2 ** 127 - 1, 1), "i128_min": (-2 ** 127 + 1, -1), "i128_under": (-2 ** 127, -1),
    "dec_max": (T38 - 2, 1), "dec_over": (T38 - 1, 1), "dec_min": (-(T38 - 2), -1), "dec_under": (-(T38 - 1), -1), "dec_cancel": (T38 - 1, -(T38 - 1)),
    "neg_pos": (-(2 ** 127), 2 ** 127), "wide": (2 ** 189, 2 ** 189), "wide_neg": (-(2 ** 189), -(2 ** 189)),
}
for _k in range(200):
    MERGES["rand%d" % _k] = (rand192(int(RNG.integers(1, 190))), rand192(int(RNG.integers(1, 190))))
# MIN / MAX of Decimal128: the signed high word, the unsigned low word
I128_PAIRS = [(0, -1), (2 ** 64, 2 ** 64 - 1), (-2 ** 64, -2 ** 64 - 1), (2 ** 63, 2 ** 63 - 1), (-2 ** 127, 2 ** 127 - 1), (5, 5), (T38 - 1, -(T38 - 1)), (2 ** 64 + 2 ** 63, 2 ** 65)]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("agg_plan")
    exe, cases = str(d / "agg_plan_check"), str(d / "cases.txt")
    with open(cases, "w") as f:
        for cls, names in CLASSES.items():
            for name in names + (["dec38_20"] if cls == "dec" else []):
                for op in (COUNT, SUM, MIN, MAX):
                    f.write("plan %s_%d flat %d %s -\n" % (name, op, op, name))
                f.write("plan %s_5 flat 5 %s %s\n" % (name, name, name))
        for name, a, b in (("sp_38", "dec38_19", "dec38_19"), ("sp_39", "dec38_19", "dec38_20"), ("sp_39r", "dec38_20", "dec38_19"), ("sp_q6", "dec15_2", "dec15_2"),
                           ("sp_i8_i64", "i8", "i64"), ("sp_f32_f64", "f32", "f64"), ("sp_int_float", "i64", "f64"), ("sp_int_dec", "i64", "dec38_0"),
                           ("sp_dec_float", "dec38_0", "f64"), ("sp_int_date", "i64", "date"), ("sp_no_col2", "i64", "-"), ("sp_missing2", "i64", "nope")):
            f.write("plan %s flat 5 %s %s\n" % (name, a, b))
        f.write("plan rows flat 0 - -\nplan rows_named flat 0 i64 -\nplan count_none flat 1 - -\nplan missing flat 2 nope -\nplan bad_op flat 6 i64 -\n")
        f.write("plan bad_op_big flat 4000000000 i64 -\nplan nested_rows nested 0 - -\nplan nested_sum nested 2 i64 -\nplan nested_count nested 1 st -\n")
        f.write("count c0 0\ncount c1 1\ncount c64 64\ncount c65 65\n")
        for name, (a, b) in MERGES.items():
            f.write("merge %s %d 0 %s %s\n" % (name, AK_SUM_DEC, " ".join(words(a)), " ".join(words(b))))
        for k, (a, b) in enumerate(I128_PAIRS):
            for is_max in (0, 1):
                f.write("merge mm%d_%d %d %d %s %s\n" % (k, is_max, AK_MINMAX_DEC, is_max, " ".join(words(a)), " ".join(words(b))))
                f.write("merge mmr%d_%d %d %d %s %s\n" % (k, is_max, AK_MINMAX_DEC, is_max, " ".join(words(b)), " ".join(words(a))))
        f.write("finish sum_null %d 0 0 0 0 0\n" % AK_SUM_INT)
        f.write("finish sum_fit %d 3 0 %s\n" % (AK_SUM_INT, " ".join(words(-2 ** 127))))
        f.write("finish sum_over %d 3 0 %s\n" % (AK_SP_INT, " ".join(words(2 ** 127))))
        f.write("finish dec_fit %d 3 0 %s\n" % (AK_SUM_DEC, " ".join(words(-(T38 - 1)))))
        f.write("finish dec_over %d 3 0 %s\n" % (AK_SP_DEC, " ".join(words(T38))))
        f.write("finish dec_sticky %d 3 1 %s\n" % (AK_SP_DEC, " ".join(words(5))))
        f.write("finish count %d 0 0 7 0 0\n" % AK_COUNT)
        f.write("finish minmax_null %d 0 0 0 0 0\n" % AK_MINMAX_INT)
        f.write("finish f64_all_nan %d 0 2 0 0 0\n" % AK_MINMAX_F64)
        f.write("finish f64_none %d 0 0 0 0 0\n" % AK_MINMAX_F64)
        f.write("finish mm_dec %d 2 0 %s\n" % (AK_MINMAX_DEC, " ".join(words(-5)[:2] + ["0"])))
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "agg_plan_check.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def plan(lines, name):
    """(status, kind, is_max, scale, fkind, message)"""
    ln = [x for x in lines if x.startswith("plan %s " % name)]
    assert len(ln) == 1, name
    head, msg = ln[0].split("\t")
    f = head.split()
    return int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), msg


def test_every_op_and_column_kind(lines):
    for cls, names in CLASSES.items():
        for name in names:
            st, kind, _, _, _, msg = plan(lines, "%s_%d" % (name, COUNT))
            assert (st, kind) == (OK, AK_COUNT), name      # COUNT takes every root column, dictionary columns included
            for op, table in ((SUM, SUM_OF), (MIN, MINMAX_OF), (MAX, MINMAX_OF), (SUM_PRODUCT, SP_OF)):
                st, kind, is_max, scale, _, msg = plan(lines, "%s_%d" % (name, op))
                want = table[cls]
                if want < 0:
                    assert st == -want and "'%s'" % name in msg, (name, op, st, msg)
                    continue
                assert (st, kind, is_max) == (OK, want, int(op == MAX)), (name, op, st, msg)
                if cls == "dec":
                    assert scale == SCALE[name] * (2 if op == SUM_PRODUCT else 1), (name, op)
                if cls == "ts" and op in (MIN, MAX):
                    assert scale == UNIT[name], name
                if cls in ("int", "date", "bool") and op in (MIN, MAX):
                    assert scale == -1, name


def test_scale_rule_and_mixed_products(lines):
    assert plan(lines, "sp_38")[:4] == (OK, AK_SP_DEC, 0, 38)
    for name in ("sp_39", "sp_39r", "dec38_20_5"):
        st, _, _, _, _, msg = plan(lines, name)
        assert st == UNSUPPORTED and "dec38_20" in msg, (name, msg)
    assert plan(lines, "sp_q6")[:4] == (OK, AK_SP_DEC, 0, 4)
    assert plan(lines, "sp_i8_i64")[:2] == (OK, AK_SP_INT) and plan(lines, "sp_f32_f64")[:2] == (OK, AK_SP_F64)
    for name, cols in (("sp_int_float", ("i64", "f64")), ("sp_int_dec", ("i64", "dec38_0")), ("sp_dec_float", ("dec38_0", "f64"))):
        st, _, _, _, _, msg = plan(lines, name)
        assert st == MISMATCHED and all("'%s'" % c in msg for c in cols), (name, msg)
    assert plan(lines, "sp_int_date")[0] == MISMATCHED and "'date'" in plan(lines, "sp_int_date")[5]
    assert plan(lines, "sp_no_col2")[0] == INVALID
    assert plan(lines, "sp_missing2")[0] == INVALID and "'nope'" in plan(lines, "sp_missing2")[5]


def test_arguments(lines):
    assert plan(lines, "rows")[:2] == (OK, AK_COUNT_ROWS) and plan(lines, "rows_named")[:2] == (OK, AK_COUNT_ROWS)
    assert plan(lines, "count_none")[0] == INVALID
    assert plan(lines, "missing")[0] == INVALID and "'nope'" in plan(lines, "missing")[5]
    assert plan(lines, "bad_op")[0] == INVALID and plan(lines, "bad_op_big")[0] == INVALID
    for name in ("nested_rows", "nested_sum", "nested_count"):
        assert plan(lines, name)[0] == UNSUPPORTED and "'st'" in plan(lines, name)[5], name
    counts = {x.split()[1]: (int(x.split()[2]), int(x.split()[3])) for x in lines if x.startswith("count ")}
    assert counts == {"c0": (INVALID, 0), "c1": (OK, 1), "c64": (OK, 64), "c65": (INVALID, 0)}


def test_merge_192_bits_against_python_ints(lines):
    got = {x.split()[1]: x.split()[2:] for x in lines if x.startswith("merge ")}
    for name, (a, b) in MERGES.items():
        total = a + b
        assert abs(total) < 2 ** 191
        assert signed(got[name][:3]) == total, name
        assert int(got[name][3]) == int(-2 ** 127 <= total < 2 ** 127), name
        assert int(got[name][4]) == int(abs(total) < T38), name
    assert [int(got[n][3]) for n in ("i128_max", "i128_over", "i128_min", "i128_under")] == [1, 0, 1, 0]
    assert [int(got[n][4]) for n in ("dec_max", "dec_over", "dec_min", "dec_under", "dec_cancel")] == [1, 0, 1, 0, 1]
    for k, (a, b) in enumerate(I128_PAIRS):
        for is_max in (0, 1):
            want = max(a, b) if is_max else min(a, b)
            for tag in ("mm", "mmr"):
                ws = got["%s%d_%d" % (tag, k, is_max)][:2]
                v = sum(int(w, 16) << (64 * j) for j, w in enumerate(ws))
                assert (v - (1 << 128) if v >> 127 else v) == want, (tag, k, is_max)


def test_finish(lines):
    got = {x.split()[1]: x.split()[2:] for x in lines if x.startswith("finish ")}
    assert got["sum_null"][:3] == [str(KIND_I128), "1", "0"]
    assert got["sum_fit"][:3] == [str(KIND_I128), "0", "0"] and signed(got["sum_fit"][3:6]) == -2 ** 127
    assert got["sum_over"][:3] == [str(KIND_I128), "0", "1"]
    assert got["dec_fit"][:3] == [str(KIND_DEC128), "0", "0"] and signed(got["dec_fit"][3:6]) == -(T38 - 1)
    assert got["dec_over"][2] == "1" and got["dec_sticky"][2] == "1"
    assert got["count"][:4] == [str(KIND_U64), "0", "0", "7"]
    assert got["minmax_null"][:3] == [str(KIND_I64), "1", "0"]
    assert got["f64_all_nan"][:2] == [str(KIND_F64), "0"] and got["f64_all_nan"][6] == "1"    # every value was NaN: NaN, not NULL
    assert got["f64_none"][:2] == [str(KIND_F64), "1"]
    assert got["mm_dec"][:3] == [str(KIND_DEC128), "0", "0"] and signed(got["mm_dec"][3:6]) == -5   # sign-extended into w[2]
