"""IN lists through the row filter's plan compiler under AddressSanitizer + UBSan on the CPU:
tests/hostcheck/filter_plan_in_check.cpp compiles orc_rust_amd/csrc/orcgpu_filter_plan.inc and orcgpu_in.inc -- the text
liborcgpu.so is built from -- into a stand-alone program that prints what became of every list given to it; here every table is
probed by the rule written down in device/filter_program.h (tests/in_model.py): every key is found, no other value is.  No GPU,
nothing loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import in_model as IM
from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import PredicateValue as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
FOP_CMP_INT, FOP_CMP_FLOAT, FOP_CMP_BOOL, FOP_CMP_STRING, FOP_CMP_DEC128, FOP_UNKNOWN, FOP_FALSE, FOP_OR, FOP_NOT, FOP_LIKE, FOP_IN = 0, 1, 2, 3, 4, 7, 9, 11, 12, 13, 14
IN_HAS_NULL, IN_NO_TABLE, IN_BOOL_FALSE, IN_BOOL_TRUE = 1, 2, 4, 8
FKIND_INT, FKIND_FLOAT, FKIND_BOOL, FKIND_STRING, FKIND_DEC128 = 0, 1, 2, 3, 5
EQ = 0
NAN = float("nan")


def token(v):
    i, bits, s = 0, 0, "-"
    if v.value is not None:
        if v.kind == PR.PV_UTF8:
            b = v.value.encode() if isinstance(v.value, str) else bytes(v.value)
            s = b.hex() or "="
        elif v.kind == PR.PV_DECIMAL128:
            s, i = int(v.value[0]).to_bytes(16, "little", signed=True).hex(), v.value[1]
        elif v.kind in (PR.PV_FLOAT32, PR.PV_FLOAT64):
            bits = struct.unpack("<Q", struct.pack("<d", float(v.value)))[0]
        else:
            i = int(v.value)
    return "%d:%d:%d:%x:%s" % (v.kind, v.value is None, i, bits, s)


RNG = np.random.default_rng(17)
INTS_5000 = [int(x) for x in RNG.integers(-2 ** 63, 2 ** 63 - 1, 5000)]
STRS_5000 = ["k%d" % x + "é" * (x % 7) for x in range(5000)]
# name -> (column, wrap, literals)
CASES = {
    "empty": ("i64", "leaf", []),
    "empty_under_not": ("i64", "not", []),
    "one": ("i64", "leaf", [V.Int64(7)]),
    "one_thrice": ("i32", "leaf", [V.Int8(7), V.Int64(7), V.Int16(7)]),
    "one_and_null": ("i64", "leaf", [V.Int64(7), V.Int64(None)]),
    "nulls": ("i64", "leaf", [V.Int64(None), V.Int8(None)]),
    "two": ("i64", "leaf", [V.Int64(7), V.Int64(-7)]),
    "edges": ("i64", "leaf", [V.Int64(-2 ** 63), V.Int64(0), V.Int64(-1), V.Int64(2 ** 63 - 1), V.Int64(0)]),
    "sixteen_i8": ("i8", "leaf", [V.Int8(x) for x in range(-8, 8)]),
    "date": ("date", "leaf", [V.Int32(10), V.Int64(-10), V.Int32(None)]),
    "ints_5000": ("i64", "leaf", [V.Int64(x) for x in INTS_5000]),
    "ints_65536": ("i64", "not", [V.Int64(x * 3) for x in range(65536)]),
    "ints_65537": ("i64", "leaf", [V.Int64(x) for x in range(65537)]),
    "same_65536": ("i16", "leaf", [V.Int16(5)] * 65536),
    "floats": ("f64", "leaf", [V.Float64(0.0), V.Float64(-0.0), V.Float64(NAN), V.Float32(0.1), V.Float64(0.1), V.Float64(float("inf")), V.Float64(float("-inf"))]),
    "float_nan": ("f32", "leaf", [V.Float32(NAN), V.Float64(NAN)]),
    "float_nan_null": ("f32", "leaf", [V.Float32(NAN), V.Float64(None)]),
    "float_zero": ("f64", "leaf", [V.Float64(-0.0), V.Float32(0.0), V.Float64(NAN)]),
    "bool_true": ("b", "leaf", [V.Boolean(True), V.Boolean(True)]),
    "bool_both": ("b", "leaf", [V.Boolean(True), V.Boolean(False)]),
    "bool_false_null": ("b", "leaf", [V.Boolean(False), V.Boolean(None)]),
    "bool_nulls": ("b", "leaf", [V.Boolean(None)]),
    "strings": ("s", "leaf", [V.Utf8(x) for x in ("", "a", "ab", "é", "a\x00", "x" * 90, "ab", "")]),
    "string_one": ("vc", "leaf", [V.Utf8("mango"), V.Utf8(b"mango")]),
    "string_empty": ("ch", "leaf", [V.Utf8("")]),
    "binary": ("bin", "leaf", [V.Utf8(b"\xff\x00"), V.Utf8(b"\x00"), V.Utf8(None)]),
    "strs_5000": ("s", "leaf", [V.Utf8(x) for x in STRS_5000]),
    "bytes_at_limit": ("s", "leaf", [V.Utf8(bytes([65 + k]) * (1 << 20)) for k in range(4)]),
    "bytes_above_limit": ("s", "leaf", [V.Utf8(bytes([65 + k]) * (1 << 20)) for k in range(4)] + [V.Utf8("b")]),
    "decimals": ("dec", "leaf", [V.Decimal128((150, 2)), V.Decimal128((15, 1)), V.Decimal128((-2, 0)), V.Decimal128((1505, 3)), V.Decimal128((10 ** 38 - 1, 0)),
                                 V.Decimal128((-(10 ** 38 - 1), 0)), V.Decimal128((0, 38))]),
    "decimal_off_scale": ("dec", "leaf", [V.Decimal128((1505, 3)), V.Decimal128((1, 38))]),
    "decimal_one": ("dec", "leaf", [V.Decimal128((1505, 3)), V.Decimal128((-1, 0))]),
    "timestamps": ("ts", "leaf", [V.TimestampNs(1000), V.TimestampNs(-1000), V.TimestampNs(1500), V.TimestampNs(-1), V.TimestampNs(0), V.TimestampNs(None)]),
    "timestamp_between": ("ts", "leaf", [V.TimestampNs(1500), V.TimestampNs(-1)]),
    "timestamp_one": ("ts", "leaf", [V.TimestampNs(1500), V.TimestampNs(-2000)]),
    # refusals
    "utf8_on_int": ("i64", "leaf", [V.Int64(1), V.Utf8("a")]),
    "null_utf8_on_int": ("i64", "leaf", [V.Int64(1), V.Utf8(None)]),
    "int8_on_date": ("date", "leaf", [V.Int32(1), V.Int8(1)]),
    "int_on_float": ("f64", "leaf", [V.Int64(1)]),
    "int_on_bool": ("b", "leaf", [V.Boolean(True), V.Int8(1)]),
    "int_on_string": ("s", "leaf", [V.Int64(1)]),
    "int_on_decimal": ("dec", "leaf", [V.Decimal128((1, 0)), V.Int64(1)]),
    "decimal_on_int": ("i64", "leaf", [V.Decimal128((1, 0))]),
    "int_on_timestamp": ("ts", "leaf", [V.Int64(1)]),
    "timestamp_as_decimal": ("ts9", "leaf", [V.TimestampNs(0), V.TimestampNs(5)]),
    "nested_column": ("i64", "nested", [V.Int64(1), V.Int64(2)]),
    "no_such_column": ("nope", "leaf", [V.Int64(1)]),
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_plan_in")
    exe, cases = str(d / "filter_plan_in_check"), str(d / "cases.txt")
    with open(cases, "w") as f:
        for name, (col, wrap, vals) in CASES.items():
            f.write(" ".join([name, col, wrap] + [token(v) for v in vals]) + "\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_plan_in_check.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def got(lines, name):
    """status alone for a refusal, else (instructions, op, cmp, i, lo, bits of f, payload bytes or None)"""
    ln = [x for x in lines if x[0] == "in" and x[1] == name]
    assert len(ln) == 1, name
    ln = ln[0]
    if len(ln) == 4:
        return int(ln[2]), int(ln[3])
    assert int(ln[2]) == OK
    payload = None if ln[12] == "-" else b"" if ln[12] == "=" else bytes.fromhex(ln[12])
    assert payload is None or len(payload) == int(ln[11])
    return int(ln[4]), int(ln[5]), int(ln[6]), int(ln[7]), int(ln[8]), int(ln[9], 16), payload


def table_of(lines, name, kind, want_keys, flags=0, want_lo=None, planes=0):
    n_insn, op, cmp_, i, lo, _, blob = got(lines, name)
    wrap = CASES[name][1]
    assert (n_insn, op, cmp_, i) == (2 if wrap == "not" else 1, FOP_IN, flags, planes), name
    assert want_lo is None or lo == want_lo
    t = IM.Table(blob)
    assert (t.kind, t.flags, t.n_keys) == (kind, flags, len(want_keys)), name
    assert sorted(t.keys()) == sorted(want_keys), name  # de-duplicated: each key once, and nothing else
    longest = 0
    for k in want_keys:
        found, steps = t.probe(k)
        assert found, (name, k)
        longest = max(longest, steps)
    assert longest <= 64, (name, longest)  # (at a load of at most one half linear probing stays short)
    return t


def test_shapes_without_a_table(lines):
    assert got(lines, "empty")[:2] == (1, FOP_FALSE)
    assert got(lines, "empty_under_not")[:2] == (2, FOP_FALSE)
    assert got(lines, "nulls")[:2] == (1, FOP_UNKNOWN) and got(lines, "bool_nulls")[:2] == (1, FOP_UNKNOWN)
    assert got(lines, "float_nan_null")[:2] == (1, FOP_UNKNOWN)
    # one distinct usable key and no NULL: the comparison EQ itself
    assert got(lines, "one")[:4] == (1, FOP_CMP_INT, EQ, 7) and got(lines, "one_thrice")[:4] == (1, FOP_CMP_INT, EQ, 7)
    assert got(lines, "same_65536")[:4] == (1, FOP_CMP_INT, EQ, 5)
    n_insn, op, cmp_, _, _, bits, _ = got(lines, "float_zero")
    assert (n_insn, op, cmp_, bits) == (1, FOP_CMP_FLOAT, EQ, 0)  # -0.0, 0.0f and a NaN: the one key 0.0
    assert got(lines, "bool_true")[:4] == (1, FOP_CMP_BOOL, EQ, 1)
    assert got(lines, "string_one")[:3] == (1, FOP_CMP_STRING, EQ) and got(lines, "string_one")[6] == b"mango"
    assert got(lines, "string_empty")[:3] == (1, FOP_CMP_STRING, EQ) and got(lines, "string_empty")[6] == b""
    n_insn, op, cmp_, hi, lo, _, _ = got(lines, "decimal_one")
    assert (n_insn, op, cmp_, hi, lo) == (1, FOP_CMP_DEC128, EQ, -1, 2 ** 64 - 100)  # -1 at scale 2; 1.505 lands on no value
    assert got(lines, "timestamp_one")[:4] == (1, FOP_CMP_INT, EQ, -2)
    # no usable key: FALSE on valid rows, without a table; a Boolean column never has one
    assert got(lines, "float_nan")[:5] == (1, FOP_IN, IN_NO_TABLE, -1, FKIND_FLOAT)
    assert got(lines, "decimal_off_scale")[:5] == (1, FOP_IN, IN_NO_TABLE, -1, FKIND_DEC128)
    assert got(lines, "timestamp_between")[:5] == (1, FOP_IN, IN_NO_TABLE, -1, FKIND_INT)
    assert got(lines, "bool_both")[:5] == (1, FOP_IN, IN_NO_TABLE | IN_BOOL_FALSE | IN_BOOL_TRUE, -1, FKIND_BOOL)
    assert got(lines, "bool_false_null")[:5] == (1, FOP_IN, IN_NO_TABLE | IN_BOOL_FALSE | IN_HAS_NULL, -1, FKIND_BOOL)


def test_every_key_is_found_and_nothing_else(lines):
    outside = [int(x) for x in RNG.integers(-2 ** 63, 2 ** 63 - 1, 300)] + [1, 6, 8, -8, 2 ** 62]
    t = table_of(lines, "two", IM.IN_KEY_I64, [7, (-7) & IM.M64], want_lo=FKIND_INT)
    assert t.n_slots == 4 and len(t.blob) <= 32768
    table_of(lines, "one_and_null", IM.IN_KEY_I64, [7], flags=IN_HAS_NULL)
    t = table_of(lines, "edges", IM.IN_KEY_I64, [1 << 63, 0, IM.M64, (1 << 63) - 1])  # every int64 is a legal key
    assert not t.probe(1)[0] and not t.probe(-2)[0]
    t = table_of(lines, "sixteen_i8", IM.IN_KEY_I64, [x & IM.M64 for x in range(-8, 8)])
    assert t.n_slots == 32 and not any(t.probe(x)[0] for x in (8, -9, 127, -128))
    table_of(lines, "date", IM.IN_KEY_I64, [10, (-10) & IM.M64], flags=IN_HAS_NULL)
    t = table_of(lines, "ints_5000", IM.IN_KEY_I64, [x & IM.M64 for x in set(INTS_5000)])
    assert t.n_slots == 16384 and len(t.blob) > 32768  # above what is staged in LDS
    assert not any(t.probe(x)[0] for x in outside if x not in set(INTS_5000))
    t = table_of(lines, "ints_65536", IM.IN_KEY_I64, [x * 3 for x in range(65536)])
    assert t.n_slots == 131072 and not any(t.probe(x)[0] for x in (1, 2, -3, 3 * 65536))
    # floats: the keys are the bits of the normalised double; the NaN is gone, the two zeros are one, 0.1f is not 0.1
    f32 = struct.unpack("<f", struct.pack("<f", 0.1))[0]
    t = table_of(lines, "floats", IM.IN_KEY_I64, [IM.float_key(x) for x in (0.0, f32, 0.1, float("inf"), float("-inf"))], want_lo=FKIND_FLOAT)
    assert t.probe(IM.float_key(-0.0))[0] and not t.probe(IM.float_key(0.2))[0]
    # strings
    words = [b"", b"a", b"ab", "é".encode(), b"a\x00", b"x" * 90]
    t = table_of(lines, "strings", IM.IN_KEY_STRING, words, want_lo=FKIND_STRING)
    assert (t.min_len, t.max_len) == (0, 90)
    assert not any(t.probe(x)[0] for x in (b"b", b"a\x00\x00", b"x" * 89, b"x" * 91, b"\x00", "è".encode()))
    t = table_of(lines, "binary", IM.IN_KEY_STRING, [b"\xff\x00", b"\x00"], flags=IN_HAS_NULL)
    assert (t.min_len, t.max_len) == (1, 2) and not t.probe(b"")[0]
    t = table_of(lines, "strs_5000", IM.IN_KEY_STRING, [x.encode() for x in STRS_5000])
    assert len(t.blob) > 32768 and not any(t.probe(("k%d" % x).encode())[0] for x in range(5000) if x % 7)
    # Decimal(.., 2): 1.50 twice, -2, the extremes; 1.505 lands on no value; 10^38 - 1 at scale 0 leaves the column's digits
    t = table_of(lines, "decimals", IM.IN_KEY_DEC128, [IM.dec128_key(x) for x in (150, -200, 0)], want_lo=FKIND_DEC128)
    assert not t.probe(IM.dec128_key(1505))[0] and not t.probe(IM.dec128_key(-150))[0]
    # Timestamp in microseconds: 1000 ns, -1000 ns and 0 land on a value, 1500 ns and -1 ns lie between two
    table_of(lines, "timestamps", IM.IN_KEY_I64, [1, (-1) & IM.M64, 0], flags=IN_HAS_NULL, want_lo=FKIND_INT)


def test_limits_and_refusals_name_the_column(lines):
    assert got(lines, "ints_65537") == (UNSUPPORTED, 1)
    t = table_of(lines, "bytes_at_limit", IM.IN_KEY_STRING, [bytes([65 + k]) * (1 << 20) for k in range(4)])
    assert t.min_len == t.max_len == 1 << 20
    assert got(lines, "bytes_above_limit") == (UNSUPPORTED, 1)
    for name in ("utf8_on_int", "null_utf8_on_int", "int8_on_date", "int_on_float", "int_on_bool", "int_on_string", "decimal_on_int"):
        assert got(lines, name) == (MISMATCHED, 1), name
    for name in ("int_on_decimal", "int_on_timestamp", "timestamp_as_decimal", "nested_column"):
        assert got(lines, name) == (UNSUPPORTED, 1), name
    assert got(lines, "no_such_column") == (INVALID, 1)


def test_malformed_node_lists_and_a_program_of_several_leaves(lines):
    bad = {ln[1]: (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "bad"}
    for name in ("literal_alone", "literal_under_and", "literal_under_not", "literal_behind_the_list", "child_is_a_comparison", "child_is_an_in",
                 "literal_with_children", "list_ends_early", "list_ends_early_in_a_tree", "nodes_behind_the_root", "no_column_name", "op_11_is_unknown"):
        assert bad[name][0] == INVALID, name
    assert bad["no_such_column"] == (INVALID, 1)
    assert bad["literal_with_a_column_is_fine"][0] == OK
    planes = [tuple(int(x) for x in p.split(":")) for p in [ln for ln in lines if ln[0] == "planes"][0][1:]]
    # IN (1, 2) -> plane 0; IN (5) -> EQ; LIKE -> plane 1; the Boolean list -> no plane; IN ('xy', 'z') -> plane 2; IN () -> FALSE
    assert planes == [(FOP_IN, 0, 0), (FOP_CMP_INT, 5, EQ), (FOP_OR, 0, 0), (FOP_LIKE, 1, 1), (FOP_OR, 0, 0),
                      (FOP_IN, -1, IN_NO_TABLE | IN_BOOL_FALSE | IN_BOOL_TRUE), (FOP_OR, 0, 0), (FOP_IN, 2, 0), (FOP_OR, 0, 0), (FOP_FALSE, 0, 0), (FOP_OR, 0, 0)]
    # the leaf lists the two plane kernels are launched over: the instruction indices of planes 0 and 2 (IN) and of plane 1 (LIKE)
    leaves = [ln for ln in lines if ln[0] == "leaves"][0]
    at = {i: k for k, (op, i, _) in enumerate(planes) if op in (FOP_IN, FOP_LIKE) and i >= 0}
    assert leaves[1] == "like" and leaves[3] == "in" and [int(x) for x in leaves[2:3]] == [at[1]] == [3] and [int(x) for x in leaves[4:]] == [at[0], at[2]] == [0, 7]
    depth = [ln for ln in lines if ln[0] == "depth"][0]
    assert [int(x) for x in depth[1:]] == [OK, INVALID]
