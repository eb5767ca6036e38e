"""The Python side of the GROUP BY limits (orc_rust_amd/aggregate.py check_group_limits, ArrowReaderBuilder.aggregate(...,
max_groups=, max_total_groups=), Context.result_aggregate_groups(..., max_groups=)): the limits are checked before anything reaches
the library, the binding declares the two entry points, and the constants are those of include/orcgpu.h.  No GPU."""
import os
import re

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = [Agg.count_rows()]
KEYS = ["k"]

# (max_groups, max_total_groups, the exception, what its message holds)
BAD = [
    (True, None, TypeError, "True"), (None, False, TypeError, "False"), (1.0, None, TypeError, "1.0"), ("300", None, TypeError, "'300'"),
    (None, [1], TypeError, "[1]"),
    (0, None, ValueError, "0"), (-1, None, ValueError, "-1"), (2 ** 20 + 1, None, ValueError, str(2 ** 20 + 1)),
    (None, 0, ValueError, "0"), (None, 2 ** 24 + 1, ValueError, str(2 ** 24 + 1)),
    (300, 299, ValueError, "299"),              # the total below the limit of one stripe
    (None, 255, ValueError, "255"),             # ... below the DEFAULT of one stripe
    (65537, None, ValueError, "65536"),         # ... the DEFAULT total below the limit that was given
]


def test_exports_and_constants():
    for name in ("orcgpu_result_aggregate_groups_limit", "orcgpu_reader_set_group_limits"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load(), name)
    assert capi.ABI_VERSION == 4                # additive: no struct changed
    hdr = open(os.path.join(ROOT, "include", "orcgpu.h")).read()
    for name, value in (("LIMIT_MAX", A.GROUP_LIMIT_MAX), ("TOTAL_LIMIT_MAX", A.GROUP_TOTAL_LIMIT_MAX), ("MAX", A.GROUP_MAX), ("MAX_TOTAL", A.GROUP_MAX_TOTAL)):
        assert re.search(r"#define ORCGPU_GROUP_%s (\d+)" % name, hdr).group(1) == str(value)
    assert (A.GROUP_LIMIT_MAX, A.GROUP_TOTAL_LIMIT_MAX) == (2 ** 20, 2 ** 24)


def test_limits_are_checked():
    for groups, total, exc, word in BAD:
        with pytest.raises(exc) as e:
            A.check_group_limits(groups, total, KEYS)
        assert word in str(e.value), (groups, total, str(e.value))
    # what passes, as the C calls take it: 0 = the default
    assert A.check_group_limits(None, None, KEYS) == (0, 0) and A.check_group_limits(None, None, None) == (0, 0)
    assert A.check_group_limits(1, None, KEYS) == (1, 0) and A.check_group_limits(256, 256, KEYS) == (256, 256)
    assert A.check_group_limits(2 ** 20, 2 ** 24, KEYS) == (2 ** 20, 2 ** 24) and A.check_group_limits(2 ** 20, 2 ** 20, KEYS) == (2 ** 20, 2 ** 20)
    assert A.check_group_limits(65536, None, KEYS) == (65536, 0) and A.check_group_limits(None, 256, KEYS) == (0, 256)
    # a limit without a group_by
    for groups, total in ((300, None), (None, 70000), (300, 70000)):
        with pytest.raises(ValueError) as e:
            A.check_group_limits(groups, total, None)
        assert "group_by" in str(e.value) and str(groups or total) in str(e.value)


def test_nothing_reaches_the_library():
    # the builder and the context check first: neither handle is touched (there is none here)
    b = ArrowReaderBuilder(None, None)
    ctx = capi.Context.__new__(capi.Context)
    ctx.h = None
    for groups, total, exc, _ in BAD:
        with pytest.raises(exc):
            b.aggregate(SPECS, group_by=KEYS, max_groups=groups, max_total_groups=total)
        with pytest.raises(exc):
            b.aggregating_reader(SPECS, group_by=KEYS, max_groups=groups, max_total_groups=total)
        if total is None and groups != 65537:   # (one result has no total to fall below)
            with pytest.raises(exc):
                ctx.result_aggregate_groups(None, SPECS, KEYS, ["k"], max_groups=groups)
    with pytest.raises(ValueError):
        b.aggregate(SPECS, max_groups=300)
    with pytest.raises(ValueError):
        b.aggregating_reader(SPECS, max_total_groups=70000)
    with pytest.raises(TypeError):              # group_by is checked as without a limit
        b.aggregate(SPECS, group_by="k", max_groups=300)
