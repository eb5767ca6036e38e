"""Decimal128 and TimestampNs literals through the row filter's plan compiler and the row-group pruning, under AddressSanitizer +
UBSan on the CPU: tests/hostcheck/filter_plan_typed_check.cpp compiles orc_rust_amd/csrc/orcgpu_filter_plan.inc,
orcgpu_decimal.inc and orcgpu_predicate.inc -- the text liborcgpu.so is built from -- into a stand-alone program that prints the
normalised (op', literal') of every case; here every line is judged with Python's integers and fractions.  No GPU, nothing
loaded into Python."""
import decimal
import os
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
EQ, NE, LT, LE, GT, GE = range(6)
FOP_CMP_INT, FOP_CMP_DEC128, FOP_UNKNOWN = 0, 4, 7
LIM = 10 ** 38
I128_MIN, I128_MAX = -2 ** 127, 2 ** 127 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
PER_UNIT = (10 ** 9, 10 ** 6, 10 ** 3, 1)


def compare(op, a, b):
    return (a == b, a != b, a < b, a <= b, a > b, a >= b)[op]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_plan_typed") / "filter_plan_typed_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_plan_typed_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def test_decimal_literals_are_normalised_to_the_column_scale(lines):
    """Every row a Decimal128 column can hold near the literal, at 0, +-1 and at +-(10^38 - 1): op'(row, literal') at the column's
    scale says what op says of the two exact rationals."""
    seen = set()
    for ln in (ln for ln in lines if ln[0] == "dec"):
        cs, u, ls, op, rc, fop, op2, lit2 = (int(x) for x in ln[1:])
        assert rc == OK and fop == FOP_CMP_DEC128, ln
        assert I128_MIN <= lit2 <= I128_MAX, ln
        x = Fraction(u * 10 ** cs, 10 ** ls)  # the literal in units of the column's scale
        fl = x.numerator // x.denominator
        d = cs - ls
        if d >= 0:
            exact = u * 10 ** d
            assert op2 == op and lit2 == max(I128_MIN, min(I128_MAX, exact)), ln  # scaled up, clamped where it leaves int128
            seen.add("d=0" if d == 0 else ("clamped" if exact != lit2 else "d>0") + ("-" if u < 0 else "+"))
            if d == 38 and ls == 0:
                seen.add("38 against 0")
        elif x.denominator == 1:
            assert (op2, lit2) == (op, fl), ln
            seen.add("r=0" + ("-" if u < 0 else "+"))
        else:
            want = {EQ: (EQ, I128_MAX), NE: (NE, I128_MAX), LT: (LE, fl), LE: (LE, fl), GT: (GT, fl), GE: (GT, fl)}[op]
            assert (op2, lit2) == want, ln
            seen.add("r!=0" + ("-" if u < 0 else "+"))
        if abs(u) == LIM - 1:
            seen.add("precision 38")
        rows = {fl + k for k in range(-2, 3)} | {lit2 - 1, lit2, lit2 + 1, 0, 1, -1, LIM - 1, 1 - LIM, 1 << 63, -(1 << 63), (1 << 64) - 1}
        for v in rows:
            if abs(v) < LIM:
                assert compare(op2, v, lit2) == compare(op, Fraction(v), x), (ln, v)
    assert seen >= {"d=0", "d>0+", "d>0-", "r=0+", "r=0-", "r!=0+", "r!=0-", "clamped+", "clamped-", "38 against 0", "precision 38"}, seen


def test_timestamp_literals_are_normalised_to_the_column_unit(lines):
    """Rows around the literal in the column's unit and at both ends of int64: op'(row, literal') says what op says of the row's
    instant in nanoseconds against the literal's."""
    n = 0
    for ln in (ln for ln in lines if ln[0] == "ts"):
        unit, ns, op, rc, fop, op2, lit2 = (int(x) for x in ln[1:])
        assert rc == OK and fop == FOP_CMP_INT and I64_MIN <= lit2 <= I64_MAX, ln
        per = PER_UNIT[unit]
        fl = ns // per  # (Python floors: -1 ns is in second -1)
        if ns % per == 0:
            assert (op2, lit2) == (op, fl), ln
        elif op in (LT, LE, GT, GE):
            assert (op2, lit2) == ((LE, fl) if op in (LT, LE) else (GT, fl)), ln
        for v in {fl - 1, fl, fl + 1, lit2, 0, -1, 1, I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX}:
            if I64_MIN <= v <= I64_MAX:
                assert compare(op2, v, lit2) == compare(op, v * per, ns), (ln, v)
        n += 1
    assert n == 4 * 17 * 6


def test_malformed_literals_and_the_type_table(lines):
    bad = {ln[1]: (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "bad"}
    for name in ("dec_15_bytes", "dec_17_bytes", "dec_no_bytes", "dec_scale_negative", "dec_scale_39", "dec_scale_huge", "dec_magnitude",
                 "dec_magnitude_negative"):
        assert bad[name] == (INVALID, 1), name
    # any other literal kind on a Decimal / Timestamp column is what it was: UNSUPPORTED, the message naming the column
    for name in ("int64_on_dec", "int64_on_ts", "timestamp_on_dec", "decimal_on_tsi", "ts_decoded_to_decimal"):
        assert bad[name] == (UNSUPPORTED, 1), name
    for name in ("decimal_on_int", "timestamp_on_string", "value_type_99"):
        assert bad[name] == (MISMATCHED, 1), name
    pair = {ln[1]: tuple(int(x) for x in ln[2:]) for ln in lines if ln[0] == "pair"}
    assert pair["dec_null_literal"] == (OK, 1, FOP_UNKNOWN) and pair["ts_null_literal"] == (OK, 1, FOP_UNKNOWN)
    assert pair["dec_ok"] == (OK, 1, FOP_CMP_DEC128) and pair["ts_ok"] == (OK, 1, FOP_CMP_INT)
    assert pair["dec_without_params"] == (OK, 1, FOP_CMP_DEC128)


def test_decimal_statistics_strings_parse_exactly(lines):
    refused = {"999999999999999999999999999999999999999", "1E+38", "<empty>", "-", ".", "abc", "1.2.3", "1e", "1e+", "12x", "_1", "1_", "1E+2000",
               "--1", "0x10"}
    got = {ln[1]: ln[2:] for ln in lines if ln[0] == "parse"}
    assert refused <= set(got) and len(got) > len(refused) + 15
    for s, (ok, unscaled, scale) in got.items():
        if s in refused:
            assert ok == "0", s
            continue
        assert ok == "1", s
        assert int(scale) >= 0 and abs(int(unscaled)) < LIM, s
        assert Fraction(int(unscaled), 10 ** int(scale)) == Fraction(decimal.Decimal(s)), (s, unscaled, scale)


def test_decimal_statistics_prune_in_exact_order(lines):
    """cmp_int's "might match" rules over [min, max] as rationals; a NOT is pushed down as the reference pushes it."""
    negate = {EQ: NE, NE: EQ, LT: GE, LE: GT, GT: LE, GE: LT}
    got = {}
    for ln in (ln for ln in lines if ln[0].startswith("stats")):
        mn, mx, op, unscaled, ls, ok, keep = ln[1], ln[2], int(ln[3]), int(ln[4]), int(ln[5]), int(ln[6]), int(ln[7])
        got[(ln[0], mn, mx, op, unscaled, ls)] = (ok, keep)
        if mn == "nine" or mx == "1.0.5" or ls == 39:
            continue
        lo, hi, v = Fraction(decimal.Decimal(mn)), Fraction(decimal.Decimal(mx)), Fraction(unscaled, 10 ** ls)
        o = negate[op] if "_not" in ln[0] else op
        want = {EQ: lo <= v <= hi, NE: not (lo == v == hi), LT: lo < v, LE: lo <= v, GT: hi > v, GE: hi >= v}[o]
        assert (ok, keep) == (1, int(want)), ln
    # what the comparison of strings gets wrong: as strings "10.0" < "9.5", so = 10.0 would drop the group, and "9.5" > "10.5", so
    # > 10.5 would keep it
    assert got[("stats", "9.5", "10.5", EQ, 100, 1)] == (1, 1)
    assert got[("stats", "9.5", "10.5", GT, 105, 1)] == (1, 0)
    assert got[("stats", "9.5", "10.5", GT, 1050, 2)] == (1, 0)
    assert got[("stats", "9.5", "10.5", LT, 9, 0)] == (1, 0) and got[("stats", "9.5", "10.5", LT, 10, 0)] == (1, 1)
    # a Timestamp leaf beside the Decimal leaf neither prunes nor fails: the Decimal leaf still drops the group
    assert got[("stats_and_ts", "9.5", "10.5", GT, 106, 1)] == (1, 0) and got[("stats_and_ts", "9.5", "10.5", EQ, 100, 1)] == (1, 1)
    # an unparsable minimum or a malformed literal fails the evaluation: the stripe is read whole
    assert got[("stats", "nine", "10.5", EQ, 100, 1)] == (0, 0)
    assert got[("stats", "9.5", "1.0.5", GT, 100, 1)] == (0, 0) and got[("stats", "9.5", "10.5", GT, 100, 39)] == (0, 0)
    assert len(got) > 150
