"""The key sets' model (tests/key_set_model.py) on hand cases whose answers are written out here: what test_gpu_key_set.py
judges the GPU by must itself say what include/orcgpu.h says."""
import numpy as np

import key_set_model as M

MIN, MAX = M.INT64_MIN, M.INT64_MAX


def tf(a):
    return a[0].tolist(), a[1].tolist()


def test_the_empty_set_is_false_everywhere_null_rows_included():
    s, has_null = M.build([], None, None)
    assert (s, has_null) == (set(), False)
    s, has_null = M.build([1, 2, 3], keep=[False, False, False])
    assert (s, has_null) == (set(), False)
    got = M.in_set([1, 2, 0], [True, True, False], s, has_null)
    assert tf(got) == ([False, False, False], [True, True, True])
    assert M.kept(got).tolist() == [] and M.kept(M.not_(got)).tolist() == [0, 1, 2]      # NOT IN the empty set keeps every row


def test_a_set_with_only_nulls_is_unknown_everywhere():
    s, has_null = M.build([0, 0], None, valid=[False, False])
    assert (s, has_null) == (set(), True)
    got = M.in_set([0, 5, 0], [True, True, False], s, has_null)
    assert tf(got) == ([False, False, False], [False, False, False])
    assert M.kept(got).tolist() == [] and M.kept(M.not_(got)).tolist() == []


def test_a_null_of_a_row_the_filter_drops_does_not_count():
    s, has_null = M.build([7, 0, 9], keep=[True, False, True], valid=[True, False, True])
    assert (s, has_null) == ({7, 9}, False)
    s, has_null = M.build([7, 0, 9], keep=[False, True, True], valid=[True, False, True])
    assert (s, has_null) == ({9}, True)


def test_the_extremes_of_int64_are_keys_like_any_other():
    s, has_null = M.build([MIN, MAX, 0, -1], None, None)
    assert s == {MIN, MAX, 0, -1} and not has_null
    got = M.in_set([MIN, MIN + 1, MAX, MAX - 1, 0, -1, 1, 0], [True] * 7 + [False], s, has_null)
    assert tf(got) == ([True, False, True, False, True, True, False, False], [False, True, False, True, False, False, True, False])
    assert M.kept(got).tolist() == [0, 2, 4, 5]


def test_duplicates_count_once():
    s, has_null = M.build([5, 5, 5, 6, 5, 6], None, None)
    assert s == {5, 6} and len(s) == 2 and not has_null
    s, has_null = M.build([5, 5, 5], None, None)
    assert s == {5}


def test_not_over_a_set_with_a_null_keeps_nothing():
    s, has_null = M.build([1, 2, 0], None, valid=[True, True, False])
    assert (s, has_null) == ({1, 2}, True)
    got = M.in_set([1, 3, 0, 2], [True, True, False, True], s, has_null)
    assert tf(got) == ([True, False, False, True], [False, False, False, False])      # the non-match 3 is UNKNOWN, not FALSE
    assert M.kept(got).tolist() == [0, 3]
    assert M.kept(M.not_(got)).tolist() == []                                         # NOT IN: nothing, as SQL's IN (subquery) requires
    # ... and without the NULL the non-match is FALSE, so NOT keeps it; the NULL row stays out either way
    got = M.in_set([1, 3, 0, 2], [True, True, False, True], s, False)
    assert M.kept(M.not_(got)).tolist() == [1]


def test_and_or_beside_a_comparison():
    s, has_null = M.build([1, 2], None, None)
    x, valid = [1, 2, 3, 0], [True, True, True, False]
    a = M.in_set(x, valid, s, has_null)
    c = M.compare(x, valid, ">", 1)
    assert M.kept(M.and_(a, c)).tolist() == [1]
    assert M.kept(M.or_(a, c)).tolist() == [0, 1, 2]
    assert M.kept(M.or_(M.not_(a), c)).tolist() == [1, 2]


def test_membership_is_isin_on_a_large_case():
    rng = np.random.default_rng(5)
    keys = rng.integers(-1000, 1000, 500)
    keep = rng.random(500) < 0.5
    s, has_null = M.build(keys, keep, None)
    assert s == set(keys[keep].tolist())
    x = rng.integers(-1200, 1200, 3000)
    got = M.in_set(x, None, s, has_null)
    assert got[0].tolist() == [int(v) in s for v in x] and got[1].tolist() == [int(v) not in s for v in x]
