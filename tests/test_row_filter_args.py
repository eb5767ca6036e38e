"""The row filter's surface, without a GPU: the builder method, the three entry points in the binding's export list, in the
header and in the library."""
import os
import re

from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReader, ArrowReaderBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orcgpu_result_filter", "orcgpu_reader_set_row_filter", "orcgpu_reader_filter_rows")


def test_the_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "orcgpu.h")).read()
    L = capi.load()
    for n in NAMES:
        assert n in capi.EXPORTS
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
        assert hasattr(L, n)
    m = re.search(r"#define ORCGPU_FILTER_MAX_DEPTH (\d+)", hdr)
    assert m and int(m.group(1)) >= 32


def test_with_row_filter_exists_and_chains():
    from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

    class FakeLib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a):
                self.calls.append(name)
                return 0
            return f

    class FakeCtx:
        def __init__(self):
            self.L = FakeLib()

        def _check(self, rc):
            assert rc == 0

    pred = P.and_([P.gt("a", V.Int64(1)), P.is_not_null("b")])
    for prune, want in ((True, ["orcgpu_reader_set_row_filter", "orcgpu_reader_set_predicate"]), (False, ["orcgpu_reader_set_row_filter"])):
        ctx = FakeCtx()
        b = ArrowReaderBuilder(ctx, 1)
        assert b.with_row_filter(pred, prune=prune) is b
        assert ctx.L.calls == want
        b._h = None
    assert callable(ArrowReader.filter_rows) and callable(capi.Context.result_filter)
