"""PredicateValue.Decimal128 / TimestampNs: what the constructors take and refuse, and how flatten() marshals the two kinds into
orcgpu_predicate_node (include/orcgpu.h: ORCGPU_PV_DECIMAL128 = 8, ORCGPU_PV_TIMESTAMP_NS = 9).  Without a GPU."""
import ctypes as C
import datetime
import decimal
import os
import re

import pytest

from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

D = decimal.Decimal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_kinds_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "orcgpu.h")).read()
    assert re.search(r"ORCGPU_PV_DECIMAL128 = (\d+)", hdr).group(1) == "8" == str(PR.PV_DECIMAL128)
    assert re.search(r"ORCGPU_PV_TIMESTAMP_NS = (\d+)", hdr).group(1) == "9" == str(PR.PV_TIMESTAMP_NS)
    assert re.search(r"#define ORCGPU_ABI_VERSION (\d+)", hdr).group(1) == "4"


def test_decimal128_takes_decimals_and_pairs():
    assert V.Decimal128(D("0.05")).value == (5, 2)
    assert V.Decimal128(D("-24")).value == (-24, 0)
    assert V.Decimal128(D("24.000")).value == (24000, 3)
    assert V.Decimal128(D("-0.0")).value == (0, 1)
    assert V.Decimal128((-55, 3)).value == (-55, 3)
    assert V.Decimal128(D(10 ** 38 - 1)).value == (10 ** 38 - 1, 0)
    assert V.Decimal128(D((1, (9,) * 38, -38))).value == (1 - 10 ** 38, 38)  # -0.99...9, all 38 digits behind the point
    assert V.Decimal128(None).value is None and V.Decimal128(None).kind == PR.PV_DECIMAL128


def test_decimal128_refuses_what_has_no_exact_scale():
    for bad in (D("1E+2"), D("NaN"), D("sNaN"), D("Infinity"), D("-Infinity"), D(10 ** 38), D((0, (1,), -39)), (10 ** 38, 0), (-10 ** 38, 5), (1, 39),
                (1, -1)):
        with pytest.raises(ValueError):
            V.Decimal128(bad)
    for bad in (1.5, "1.5", (1.0, 2), (1, 2.0), (True, 1)):
        with pytest.raises((TypeError, ValueError)):
            V.Decimal128(bad)


def test_timestamp_ns_takes_ints_and_datetimes_exactly():
    assert V.TimestampNs(-1).value == -1
    assert V.TimestampNs(datetime.datetime(1970, 1, 1)).value == 0
    # microseconds map to exact nanoseconds (a float of seconds would not hold them: 2262's seconds need 34 bits, plus 20 for the us)
    assert V.TimestampNs(datetime.datetime(2262, 4, 11, 23, 47, 16, 854775)).value == 9223372036854775000
    assert V.TimestampNs(datetime.datetime(2020, 2, 29, 12, 0, 0, 123457)).value == 1582977600123457000
    assert V.TimestampNs(datetime.datetime(1969, 12, 31, 23, 59, 59, 999999)).value == -1000
    assert V.TimestampNs(datetime.datetime(1677, 9, 21, 0, 12, 43, 145225)).value == -9223372036854775000
    # a naive datetime is wall clock; an aware one is converted to UTC
    plus2 = datetime.timezone(datetime.timedelta(hours=2))
    assert V.TimestampNs(datetime.datetime(2020, 1, 1, 2, 0, tzinfo=plus2)).value == V.TimestampNs(datetime.datetime(2020, 1, 1)).value
    assert V.TimestampNs(datetime.datetime(2020, 1, 1, tzinfo=datetime.timezone.utc)).value == 1577836800 * 10 ** 9
    assert V.TimestampNs(None).value is None and V.TimestampNs(None).kind == PR.PV_TIMESTAMP_NS
    for bad in (2 ** 63, -2 ** 63 - 1, datetime.datetime(2262, 4, 12), datetime.datetime(1677, 9, 20)):
        with pytest.raises(ValueError):
            V.TimestampNs(bad)
    for bad in (1.5, "2020-01-01", datetime.date(2020, 1, 1), True):
        with pytest.raises(TypeError):
            V.TimestampNs(bad)


def test_flatten_marshals_the_two_kinds():
    pred = P.and_([P.lt("q", V.Decimal128(D("-0.055"))), P.gte("t", V.TimestampNs(-5)), P.eq("q", V.Decimal128(None)), P.ne("t", V.TimestampNs(None)),
                   P.eq("q", V.Decimal128((10 ** 38 - 1, 0)))])
    nodes, keep = pred.flatten()
    assert len(nodes) == 6 and nodes[0].op == PR.AND and nodes[0].n_children == 5
    dec, ts, dec_null, ts_null, big = nodes[1:]

    def bytes16(n):
        # (reading the c_char_p field would stop at the first zero byte: take the pointer itself)
        return C.string_at(C.c_void_p.from_buffer(n, PR.PredicateNode.s.offset).value, 16) if n.s_len else None

    assert (dec.op, dec.column, dec.value_type, dec.value_is_null, dec.i, dec.s_len) == (PR.LT, b"q", 8, 0, 3, 16)
    assert int.from_bytes(bytes16(dec), "little", signed=True) == -55
    assert (ts.op, ts.column, ts.value_type, ts.value_is_null, ts.i, ts.s_len) == (PR.GE, b"t", 9, 0, -5, 0)
    assert (dec_null.value_type, dec_null.value_is_null, dec_null.s_len) == (8, 1, 0)
    assert (ts_null.value_type, ts_null.value_is_null, ts_null.i) == (9, 1, 0)
    assert int.from_bytes(bytes16(big), "little", signed=True) == 10 ** 38 - 1 and big.i == 0
    assert any(isinstance(k, bytes) and len(k) == 16 for k in keep)  # the 16 bytes are kept alive with the node list
