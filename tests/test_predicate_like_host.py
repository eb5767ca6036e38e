"""Row-group pruning under a LIKE leaf (orcgpu_predicate_row_groups, host only): real protobuf row-index bytes
(tests/predicate_model.py) with known minimum and maximum strings; the kept set is the rule of tests/like_model.py (might_match):
a group might match a pattern with the literal prefix p iff its upper bound >= p and its lower bound < succ(p)."""
import predicate_model as PM
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from test_predicate_host import evaluate

import like_model as LM


class Raw(str):
    """bytes where predicate_model.column_statistics takes a str and encodes it: encode() gives the bytes back"""

    def __new__(cls, b):
        self = super().__new__(cls, b.decode("latin-1"))
        self.raw = bytes(b)
        return self

    def encode(self, *args):
        return self.raw


def strings(*groups, exact=True):
    """RowIndex of a string column: groups = (min, max) as str or bytes, or None (an entry without statistics)"""
    lo, up = ("minimum", "maximum") if exact else ("lower_bound", "upper_bound")
    text = lambda v: Raw(v) if isinstance(v, bytes) else v
    return PM.row_index([None if g is None else PM.column_statistics(10, False, string={lo: text(g[0]), up: text(g[1])}) for g in groups])


GROUPS = [("", "a"), ("a", "ab"), ("ab", "ab"), ("aba", "abz"), ("abc", "abd"), ("ab\xff", "ac"), ("ac", "b"), ("b", "zz"), ("a", "zz"), ("abcd", "abcd")]


def test_prefix_patterns_keep_the_groups_the_rule_keeps():
    for exact in (True, False):  # truncated bounds are bounds: the same answers
        cols = {"s": (strings(*GROUPS, exact=exact), None)}
        dropped = 0
        for pattern in ("ab%", "ab_", "abc%x", "a%", "abcd%", "abcde%", "abcdefgh_", "b%b", "z%", "zzz%", "ab\\%%", "a_c"):
            got = evaluate(P.like("s", pattern, escape="\\"), cols, 10 * len(GROUPS), 10)
            want = [LM.might_match(lo.encode(), up.encode(), pattern.encode(), 0x5C) for lo, up in GROUPS]
            assert got == want, (pattern, exact, got, want)
            dropped += want.count(False)
        assert dropped > 30
    # the rule, spelled out on one group: values in ["abc", "abd"]
    one = {"s": (strings(("abc", "abd")), None)}
    keeps = lambda pattern: evaluate(P.like("s", pattern), one, 10, 10) == [True]
    assert keeps("ab%") and keeps("abc%") and keeps("abd%") and keeps("abcz%") and keeps("a_") and keeps("abd_")
    assert not keeps("abe%") and not keeps("abb%") and not keeps("b%") and not keeps("aa_") and not keeps("abda%")


def test_a_prefix_that_ends_in_0xff_and_one_longer_than_the_bounds():
    groups = [(b"a\xfe", b"a\xff"), (b"a\xff", b"a\xff\xff"), (b"a\xff\x01", b"b"), (b"b", b"c"), (b"\xff", b"\xff\xff\x01"), (b"\xfe", b"\xff")]
    cols = {"s": (strings(*groups), None)}
    for pattern in (b"a\xff%", b"a\xff\xff_", b"\xff%", b"\xff\xff%", b"\xff\xff\xff%", b"a\xff\x01\x01%"):
        got = evaluate(P.like("s", pattern), cols, 10 * len(groups), 10)
        want = [LM.might_match(lo, up, pattern) for lo, up in groups]
        assert got == want, (pattern, got, want)
    assert LM.succ(b"a\xff") == b"b" and LM.succ(b"\xff\xff") is None
    # succ(a 0xFF) = b: the group that starts at b is out, the one that ends at a 0xFF 0xFF is in
    assert evaluate(P.like("s", b"a\xff%"), cols, 60, 10) == [True, True, True, False, False, False]
    # a prefix of only 0xFF has no successor: the upper bound alone decides
    assert evaluate(P.like("s", b"\xff\xff%"), cols, 60, 10) == [False, False, False, False, True, False]
    # a prefix longer than both bounds
    short = {"s": (strings(("ab", "ab"), ("ab", "abd"), ("abc", "abc")), None)}
    assert evaluate(P.like("s", "abcd%"), short, 30, 10) == [False, True, False]


def test_what_keeps_everything_and_never_fails():
    cols = {"s": (strings(("abc", "abd"), ("x", "y"), None), None)}
    every = [True, True, True]
    for pred in (P.not_like("s", "q%"), P.not_(P.not_(P.not_like("s", "q%"))), P.like("s", "%q"), P.like("s", "_q%"), P.like("s", "%"), P.like("s", None),
                 P.like("s", "q%!", escape="!"),  # malformed: the row filter's error to report, not the pruning's
                 P.like("nope", "q%")):
        assert evaluate(pred, cols, 30, 10) == every
    assert evaluate(P.like("s", "q%"), cols, 30, 10) == [False, False, True]  # (the entry without statistics stays)
    assert evaluate(P.not_(P.not_(P.like("s", "q%"))), cols, 30, 10) == [False, False, True]
    # other statistics kinds say nothing, and a group without typed statistics does not fail the evaluation as a comparison does
    ints = {"s": (PM.row_index([PM.column_statistics(10, False, integer=(1, 2)), PM.column_statistics(0, True)]), None)}
    assert evaluate(P.like("s", "q%"), ints, 20, 10) == [True, True]
    assert evaluate(P.gt("s", V.Utf8("q")), ints, 20, 10) == 10
    # inside AND / OR the leaf combines like any other
    both = {"s": (strings(("abc", "abd"), ("x", "y")), None), "t": (strings(("k", "l"), ("k", "l")), None)}
    assert evaluate(P.and_([P.like("s", "ab%"), P.like("t", "k%")]), both, 20, 10) == [True, False]
    assert evaluate(P.or_([P.like("s", "ab%"), P.like("t", "m%")]), both, 20, 10) == [True, False]
    assert evaluate(P.not_(P.or_([P.like("s", "ab%"), P.like("t", "m%")])), both, 20, 10) == [True, True]


def test_a_pattern_without_a_wildcard_is_eq_with_the_bloom_filter():
    words = PM.bloom_index([PM.bloom_with([PM.murmur3_64(b"alpha"), PM.murmur3_64(b"ga%ma")], 3, 4)], utf8=True)
    names = {"name": (strings(("alpha", "gamma")), words)}
    assert evaluate(P.like("name", "alpha"), names, 10, 10) == [True]
    assert evaluate(P.like("name", "beta"), names, 10, 10) == [False]          # inside the bounds: the Bloom filter says no
    assert evaluate(P.eq("name", V.Utf8("beta")), names, 10, 10) == [False]    # ... as EQ does
    assert evaluate(P.like("name", "zeta"), names, 10, 10) == [False]          # outside the bounds
    assert evaluate(P.like("name", "ga\\%ma", escape="\\"), names, 10, 10) == [True]   # the unescaped literal is what is hashed
    assert evaluate(P.like("name", "ga\\%ma"), names, 10, 10) == [True]        # (without an escape a wildcard: prefix "ga\")
    assert evaluate(P.like("name", "bet%"), names, 10, 10) == [True]           # a prefix pattern never asks the filter
    assert evaluate(P.not_like("name", "beta"), names, 10, 10) == [True]
    # truncated bounds equal to the literal: EQ's own rule (the actual minimum lies above a truncated lower bound)
    trunc = {"name": (strings(("alpha", "gamma"), exact=False), None)}
    for lit in ("alpha", "gamma", "beta"):
        assert evaluate(P.like("name", lit), trunc, 10, 10) == evaluate(P.eq("name", V.Utf8(lit)), trunc, 10, 10)
