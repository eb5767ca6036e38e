"""The row filter's model (tests/filter_model.py) pinned by hand-written truth tables and cross-checked against pyarrow.compute:
what the GPU tests judge the kernels by has to be right by itself.  No GPU."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import filter_model as FM
from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

T, F, U = "T", "F", "U"


def tv(pair):
    t, f = pair
    assert not (t & f).any()
    return [T if a else (F if b else U) for a, b in zip(t, f)]


# a column x: 1 where TRUE is wanted, 0 where FALSE, null where UNKNOWN -- `x = 1` is then T / F / U by row
def three(values):
    return pa.array([{T: 1, F: 0, U: None}[v] for v in values], pa.int32())


X = P.eq("x", V.Int32(1))
Y = P.eq("y", V.Int32(1))
PAIRS = [(a, b) for a in (T, F, U) for b in (T, F, U)]
TABLE = pa.table({"x": three([a for a, _ in PAIRS]), "y": three([b for _, b in PAIRS])})


def test_truth_tables_of_and_or_not():
    assert tv(FM.evaluate(X, TABLE)) == [a for a, _ in PAIRS]
    #                 TT TF TU FT FF FU UT UF UU
    assert tv(FM.evaluate(P.and_([X, Y]), TABLE)) == [T, F, U, F, F, F, U, F, U]
    assert tv(FM.evaluate(P.or_([X, Y]), TABLE)) == [T, T, T, T, F, U, T, U, U]
    assert tv(FM.evaluate(P.not_(X), TABLE)) == [F, F, F, T, T, T, U, U, U]
    assert tv(FM.evaluate(P.not_(P.not_(X)), TABLE)) == [a for a, _ in PAIRS]


def test_empty_and_is_true_empty_or_is_false():
    assert tv(FM.evaluate(P.and_([]), TABLE)) == [T] * 9
    assert tv(FM.evaluate(P.or_([]), TABLE)) == [F] * 9
    assert tv(FM.evaluate(P.not_(P.and_([])), TABLE)) == [F] * 9


def test_null_tests_are_never_unknown_and_a_null_literal_always_is():
    assert tv(FM.evaluate(P.is_null("x"), TABLE)) == [F, F, F, F, F, F, T, T, T]
    assert tv(FM.evaluate(P.is_not_null("x"), TABLE)) == [T, T, T, T, T, T, F, F, F]
    for op in range(6):
        assert tv(FM.evaluate(P.comparison("x", op, V.Int32(None)), TABLE)) == [U] * 9
    assert FM.keep_mask(P.not_(P.eq("x", V.Int32(None))), TABLE).sum() == 0


def test_nan_and_signed_zero_follow_ieee():
    nan = float("nan")
    t = pa.table({"f": pa.array([nan, 0.0, -0.0, 1.0, None], pa.float64())})
    want = {PR.EQ: [F, F, F, F, U], PR.NE: [T, T, T, T, U], PR.LT: [F, F, F, F, U], PR.LE: [F, F, F, F, U], PR.GT: [F, F, F, F, U], PR.GE: [F, F, F, F, U]}
    for op, w in want.items():
        assert tv(FM.evaluate(P.comparison("f", op, V.Float64(nan)), t)) == w, op
    assert tv(FM.evaluate(P.eq("f", V.Float64(0.0)), t)) == [F, T, T, F, U]
    assert tv(FM.evaluate(P.eq("f", V.Float64(-0.0)), t)) == [F, T, T, F, U]
    assert tv(FM.evaluate(P.lt("f", V.Float64(0.0)), t)) == [F, F, F, F, U]
    assert tv(FM.evaluate(P.ne("f", V.Float64(1.0)), t)) == [T, T, T, F, U]
    # a Float32 literal is rounded through float first: 0.1f is not 0.1
    t32 = pa.table({"f": pa.array([np.float32(0.1)], pa.float32())})
    assert tv(FM.evaluate(P.eq("f", V.Float32(0.1)), t32)) == [T]
    assert tv(FM.evaluate(P.eq("f", V.Float64(0.1)), t32)) == [F]


def test_strings_order_by_unsigned_byte():
    t = pa.table({"b": pa.array([b"\x7f", b"\x80", b"", b"ab", b"abc", None], pa.binary())})
    assert tv(FM.evaluate(P.lt("b", V.Utf8(b"\x80")), t)) == [T, F, T, T, T, U]     # 0x7f < 0x80: unsigned
    assert tv(FM.evaluate(P.lt("b", V.Utf8(b"abc")), t)) == [F, F, T, T, F, U]      # a prefix sorts before the longer string
    assert tv(FM.evaluate(P.gte("b", V.Utf8(b"")), t)) == [T, T, T, T, T, U]        # nothing sorts before the empty string
    assert tv(FM.evaluate(P.eq("b", V.Utf8(b"")), t)) == [F, F, T, F, F, U]
    s = pa.table({"s": pa.array(["é", "z", "", None])})
    assert tv(FM.evaluate(P.gt("s", V.Utf8("z")), s)) == [T, F, F, U]               # 0xc3 0xa9 > 'z'


def test_refusals_of_the_type_table():
    t = FM.make_table(5)
    for pred, code in ((P.eq("s", V.Int32(1)), 6), (P.eq("i32", V.Utf8("1")), 6), (P.eq("d", V.Int8(1)), 6), (P.eq("b", V.Int32(1)), 6),
                       (P.lt("ts", V.Int64(0)), 7), (P.lt("dec", V.Int64(0)), 7), (P.eq("nope", V.Int32(1)), 101), (P.is_null("nope"), 101)):
        with pytest.raises(FM.FilterRefused) as e:
            FM.evaluate(pred, t)
        assert e.value.code == code
    assert FM.keep_mask(P.is_null("ts"), t).sum() + FM.keep_mask(P.is_not_null("ts"), t).sum() == 5


PC_OPS = {PR.EQ: pc.equal, PR.NE: pc.not_equal, PR.LT: pc.less, PR.LE: pc.less_equal, PR.GT: pc.greater, PR.GE: pc.greater_equal}


def pc_eval(pred, table):
    """The same predicate as a nullable Boolean array of pyarrow.compute."""
    n = table.num_rows
    if pred.op == PR.AND:
        acc = pa.array([True] * n)
        for c in pred.children:
            acc = pc.and_kleene(acc, pc_eval(c, table))
        return acc
    if pred.op == PR.OR:
        acc = pa.array([False] * n)
        for c in pred.children:
            acc = pc.or_kleene(acc, pc_eval(c, table))
        return acc
    if pred.op == PR.NOT:
        return pc.invert(pc_eval(pred.children[0], table))
    col = table.column(pred.column).combine_chunks()
    if pred.op == PR.IS_NULL:
        return pc.is_null(col)
    if pred.op == PR.IS_NOT_NULL:
        return pc.is_valid(col)
    lit = pred.value.value
    if pa.types.is_date32(col.type):
        col = col.cast(pa.int32())
    if pa.types.is_string(col.type):
        col = col.cast(pa.binary())  # (pyarrow compares binaries by unsigned byte)
    if lit is None:
        return pa.array([None] * n, pa.bool_())
    if pred.value.kind == PR.PV_UTF8:
        lit = lit.encode() if isinstance(lit, str) else lit
    if pred.value.kind == PR.PV_FLOAT32:
        lit = float(np.float32(lit))
    if pa.types.is_floating(col.type):
        col = col.cast(pa.float64())
    return PC_OPS[pred.op](col, pa.scalar(lit, col.type))


def test_the_model_agrees_with_pyarrow_compute_on_the_truth_tables():
    for pred in (X, P.and_([X, Y]), P.or_([X, Y]), P.not_(X), P.and_([]), P.or_([]), P.is_null("x"), P.eq("x", V.Int32(None)),
                 P.not_(P.or_([P.and_([X, P.not_(Y)]), P.is_null("y")]))):
        t, f = FM.evaluate(pred, TABLE)
        got = pc_eval(pred, TABLE).to_pylist()
        assert got == [True if a else (False if b else None) for a, b in zip(t, f)]


@pytest.fixture(scope="module")
def table():
    return FM.make_table(4097)


@pytest.fixture(scope="module")
def fuzz(table):
    return FM.random_predicates(table, 200)


def test_the_model_agrees_with_pyarrow_compute_on_the_fuzz_predicates(table, fuzz):
    for pred in fuzz:
        t, f = FM.evaluate(pred, table)
        want = pc_eval(pred, table)
        assert want.to_pylist() == [True if a else (False if b else None) for a, b in zip(t, f)]
        kept = table.filter(want, null_selection_behavior="drop")
        assert kept.column("id").to_pylist() == FM.filter_table(table, pred).column("id").to_pylist()


def test_the_fuzz_generator_is_not_trivial(table, fuzz):
    """At least a quarter of the 200 predicates keep some but not all rows (the GPU test asserts the same count)."""
    assert len(fuzz) == 200 and max(FM.depth(p) for p in fuzz) <= 3
    partial = sum(0 < FM.keep_mask(p, table).sum() < table.num_rows for p in fuzz)
    print("predicates that keep some but not all rows:", partial)
    assert partial >= 50


def test_rebatch_and_expected_batches():
    t = FM.make_table(10)
    assert [b.num_rows for b in FM.rebatch(t, [4, 0, 6], 4)] == [4, 4, 2]
    assert [b.column("id").to_pylist() for b in FM.rebatch(t, [3, 7], 5)] == [[0, 1, 2], [3, 4, 5, 6, 7], [8, 9]]
    pred = P.gte("id", V.Int64(2))
    got = FM.expected_batches(t, pred, [4, 6], 3)
    assert [b.column("id").to_pylist() for b in got] == [[2, 3], [4, 5, 6], [7, 8, 9]]
    got = FM.expected_batches(t, pred, [4, 6], 3, [[(1, 2)], None])
    assert [b.column("id").to_pylist() for b in got] == [[2], [4, 5, 6], [7, 8, 9]]
    assert FM.expected_batches(t, P.lt("id", V.Int64(0)), [4, 6], 3) == []
