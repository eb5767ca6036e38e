"""ArrowReaderBuilder.with_computed_columns: the arguments it refuses before anything reaches the GPU, what the header and the
bindings declare, and that a builder on which it is not called is what it was.  No GPU."""
import os

import pytest

from orc_rust_amd import arrow_reader as R
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, lit
from orc_rust_amd.arrow_reader import ArrowReader, ArrowReaderBuilder, check_computed_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_and_the_bindings_declare_it():
    with open(os.path.join(ROOT, "include", "orcgpu.h")) as f:
        header = f.read()
    for text in ("#define ORCGPU_COMPUTED_MAX 8", "Computed columns",
                 "int orcgpu_reader_set_computed_columns(orcgpu_reader* r, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n);",
                 "int orcgpu_reader_computed_overflow_rows(const orcgpu_reader* r, uint64_t* rows);"):
        assert text in header, text
    assert R.COMPUTED_MAX == 8
    for name in ("orcgpu_reader_set_computed_columns", "orcgpu_reader_computed_overflow_rows"):
        assert name in capi.EXPORTS
    assert callable(ArrowReaderBuilder.with_computed_columns) and callable(ArrowReader.computed_overflow_rows)


def test_accepted_forms():
    e = col("a") * (1 - col("b"))
    assert check_computed_columns({"r": e}) == [("r", e)]
    assert check_computed_columns([("r", e), ("s", col("a") + 1)])[1][0] == "s"
    assert check_computed_columns((("r", e),)) == [("r", e)]
    assert len(check_computed_columns([("c%d" % k, col("a") + k) for k in range(8)])) == 8


@pytest.mark.parametrize("columns, error, fragment", [
    ("r", TypeError, "a dict {name: Expr} or a list"),
    (None, TypeError, "a dict {name: Expr} or a list"),
    ({"r"}, TypeError, "a dict {name: Expr} or a list"),
    ([("r",)], TypeError, "(name, Expr) pair"),
    (["r"], TypeError, "(name, Expr) pair"),
    ([(1, col("a"))], TypeError, "a column name must be a str"),
    ({b"r": col("a")}, TypeError, "a column name must be a str"),
    ([("r", "a + b")], TypeError, "is an aggregate.Expr"),
    ([("r", Agg.sum("a"))], TypeError, "is an aggregate.Expr"),
    ([("r", 1)], TypeError, "is an aggregate.Expr"),
    ([("", col("a"))], ValueError, "an empty column name"),
    ([("r", col("a")), ("r", col("b"))], ValueError, "'r' is given twice"),
    ([], ValueError, "no computed column given"),
    ({}, ValueError, "no computed column given"),
    ([("c%d" % k, col("a") + k) for k in range(9)], ValueError, "9 computed columns, at most 8"),
])
def test_refusals(columns, error, fragment):
    with pytest.raises(error) as e:
        check_computed_columns(columns)
    assert fragment in str(e.value)


def test_node_count_past_32():
    e = col("a")
    for _ in range(16):
        e = e + lit(1)
    assert e.node_count() == 33
    with pytest.raises(ValueError) as err:
        check_computed_columns({"r": e})
    assert "33 nodes, at most 32" in str(err.value)
    e32 = col("a") * col("b")
    for _ in range(14):
        e32 = e32 + lit(1)
    assert e32.node_count() == 31
    assert check_computed_columns({"r": e32}) == [("r", e32)]


def test_refused_before_the_library_is_called():
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)

    class Ctx:
        L = NoLibrary()

        def _check(self, rc):
            raise AssertionError("the library was called")

    b = ArrowReaderBuilder(Ctx(), None)
    for bad in ("r", [], [("", col("a"))], [("r", 1)]):
        with pytest.raises((TypeError, ValueError)):
            b.with_computed_columns(bad)


def test_builder_is_unchanged_when_not_called():
    b = ArrowReaderBuilder(None, None)
    assert vars(b) == {"_ctx": None, "_h": None, "_keep": None, "_device_output": False}
