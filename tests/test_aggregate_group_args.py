"""The Python side of GROUP BY (orc_rust_amd/aggregate.py, ArrowReaderBuilder.aggregate(group_by=...),
Context.result_aggregate_groups): group_by is checked before anything reaches the library, the binding declares the entry points,
and the C key records become the Python keys the documentation promises.  No GPU."""
import decimal
import os
import re

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = [Agg.count_rows()]


def test_exports_and_limits():
    for name in ("orcgpu_result_aggregate_groups", "orcgpu_reader_set_group_by", "orcgpu_reader_aggregate_groups", "orcgpu_groups_count",
                 "orcgpu_groups_key", "orcgpu_groups_value", "orcgpu_groups_free"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load(), name)
    assert capi.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "orcgpu.h")).read()
    for name, value in (("MAX_KEYS", A.GROUP_MAX_KEYS), ("MAX", A.GROUP_MAX), ("MAX_TOTAL", A.GROUP_MAX_TOTAL), ("KEY_BYTES", A.GROUP_KEY_BYTES)):
        assert re.search(r"#define ORCGPU_GROUP_%s (\d+)" % name, hdr).group(1) == str(value)
    assert (A.GROUP_MAX_KEYS, A.GROUP_MAX, A.GROUP_MAX_TOTAL, A.GROUP_KEY_BYTES) == (4, 256, 65536, 64)
    assert C_sizeof_key() == 16 + 16 + 64


def C_sizeof_key():
    import ctypes
    return ctypes.sizeof(A.GroupKey)


BAD = [("abc", TypeError), (None, None), (3, TypeError), ({"a"}, TypeError), ([1], TypeError), (["a", None], TypeError), ([b"a"], TypeError),
       ([""], ValueError), (["a", ""], ValueError), (["a", "b", "a"], ValueError), (["a", "b", "c", "d", "e"], ValueError), ([], ValueError), ((), ValueError)]


def test_group_by_is_checked():
    for bad, exc in BAD:
        if exc is None:
            continue
        with pytest.raises(exc):
            A.check_group_by(bad)
    assert A.check_group_by(["a"]) == ["a"] and A.check_group_by(("a", "b", "c", "d")) == ["a", "b", "c", "d"]
    arr = A.key_array(["l_returnflag", "é"])
    assert list(arr) == [b"l_returnflag", "é".encode()]


def test_nothing_reaches_the_library():
    # the builder and the context check first: neither handle is touched (there is none here)
    b = ArrowReaderBuilder(None, None)
    ctx = capi.Context.__new__(capi.Context)
    ctx.h = None
    for bad, exc in BAD:
        if exc is None:
            continue
        with pytest.raises(exc):
            b.aggregate(SPECS, group_by=bad)
        with pytest.raises(exc):
            b.aggregating_reader(SPECS, group_by=bad)
        with pytest.raises(exc):
            ctx.result_aggregate_groups(None, SPECS, bad, ["a"])
    with pytest.raises(ValueError):          # the specs are checked as without group_by
        b.aggregate([], group_by=["a"])
    with pytest.raises(TypeError):
        ctx.result_aggregate_groups(None, [1], ["a"], ["a"])


def key(kind, w=(0, 0), is_null=0, scale_or_unit=-1, data=b""):
    k = A.GroupKey()
    k.kind, k.is_null, k.scale_or_unit, k.len = kind, is_null, scale_or_unit, len(data)
    for i in range(2):
        k.w[i] = w[i] & (2 ** 64 - 1)
    for i, x in enumerate(data[:64]):
        k.bytes[i] = x
    return k


def test_keys():
    assert A.key_of(key(A.GROUP_KEY_I64, (-3, -1))) == -3 and type(A.key_of(key(A.GROUP_KEY_I64, (7, 0)))) is int
    ts = A.key_of(key(A.GROUP_KEY_I64, (5, 0), scale_or_unit=2))
    assert ts == 5 and ts.units == "us"
    assert A.key_of(key(A.GROUP_KEY_BOOL, (1, 0))) is True and A.key_of(key(A.GROUP_KEY_BOOL)) is False
    big = -(10 ** 38 - 1)
    got = A.key_of(key(A.GROUP_KEY_DEC128, (big, big >> 64), scale_or_unit=2))
    assert isinstance(got, decimal.Decimal) and got == decimal.Decimal(big).scaleb(-2, decimal.Context(prec=60))
    assert A.key_of(key(A.GROUP_KEY_STRING, data="né".encode())) == "né" and A.key_of(key(A.GROUP_KEY_STRING)) == ""
    assert A.key_of(key(A.GROUP_KEY_STRING, data=b"\xff\xfe")) == b"\xff\xfe"
    assert A.key_of(key(A.GROUP_KEY_STRING, data=b"x" * 64)) == "x" * 64
    for kind in range(4):
        assert A.key_of(key(kind, is_null=1)) is None
