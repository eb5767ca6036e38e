"""The model of tests/key_map_model.py on hand cases: what a key map holds and what a probe answers, written out by hand."""
import pytest

import key_map_model as M


def test_build_keeps_the_kept_rows_and_their_values():
    keys = [5, 7, None, 9, 11]
    rows = [(50, 0.5), (70, None), (1, 1.0), (90, 9.0), (110, 1.5)]
    m, has_null = M.build(keys, rows, kept=[True, True, True, False, True])
    assert m == {5: (50, 0.5), 7: (70, None), 11: (110, 1.5)} and has_null
    m, has_null = M.build(keys, rows, kept=[True, True, False, True, True])
    assert 9 in m and not has_null  # (the NULL key was not kept)


def test_a_null_key_holds_no_values_and_never_matches():
    m, has_null = M.build([None, None], [(1,), (2,)])
    assert m == {} and has_null
    assert M.probe(m, [None, 1], 0) == [None, None]


def test_a_duplicate_is_refused_only_among_the_kept_rows():
    keys, rows = [1, 2, 1], [(10,), (20,), (30,)]
    with pytest.raises(M.Duplicate):
        M.build(keys, rows)
    m, _ = M.build(keys, rows, kept=[True, True, False])
    assert m == {1: (10,), 2: (20,)}
    with pytest.raises(M.Duplicate):
        M.build([M.SENTINEL, M.SENTINEL], [(1,), (2,)])


def test_max_keys():
    M.build(range(4), [(k,) for k in range(4)], max_keys=4)
    with pytest.raises(OverflowError):
        M.build(range(5), [(k,) for k in range(5)], max_keys=4)


def test_the_three_ways_a_probe_row_becomes_null():
    m, _ = M.build([1, 2, M.SENTINEL], [(10, None), (None, 2.5), (77, 7.5)])
    keys = [1, 2, 3, None, M.SENTINEL, M.SENTINEL + 1]
    assert M.probe(m, keys, 0) == [10, None, None, None, 77, None]
    assert M.probe(m, keys, 1) == [None, 2.5, None, None, 7.5, None]
    assert [M.why_null(m, k, 0) for k in keys] == [None, "value", "absent", "key", None, "absent"]
    assert [M.why_null(m, k, 1) for k in keys] == ["value", None, "absent", "key", None, "absent"]


def test_the_sentinels_value_is_a_key_like_any_other():
    assert M.SENTINEL == int.from_bytes(b"\x80" * 8, "little", signed=True)
    m, _ = M.build([M.SENTINEL], [(None,)])
    assert M.probe(m, [M.SENTINEL], 0) == [None] and M.why_null(m, M.SENTINEL, 0) == "value"  # a NULL value under a present key
    m, _ = M.build([M.INT64_MIN, M.INT64_MAX, 0], [(1,), (2,), (3,)])
    assert M.probe(m, [M.SENTINEL, M.INT64_MIN, M.INT64_MAX, 0], 0) == [None, 1, 2, 3]


def test_floats_compare_by_bits():
    assert M.bits(-0.0) == 1 << 63 and M.bits(0.0) == 0 and M.bits(0.1 + 0.2) == 0x3FD3333333333334
