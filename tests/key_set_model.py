"""A plain model of the key sets (include/orcgpu.h, "key sets"): what the build side leaves, and what `x IN SET s` says of every
probe row under SQL's three-valued logic.  numpy and Python sets, nothing of the library.

A truth value over n rows is a pair (T, F) of boolean arrays -- the rows where it is TRUE and where it is FALSE; neither: UNKNOWN.
A row filter keeps the rows where its root is TRUE."""
import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def build(keys, keep=None, valid=None):
    """The build rows' keys (ints; whatever stands in a NULL row's slot is ignored), the rows the selection and the filter keep
    (None: all) and the rows whose key is not NULL (None: all) -> (the set of distinct non-NULL keys of kept rows as a Python set,
    has_null: a kept row's key was NULL)."""
    n = len(keys)
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    assert len(keep) == n and len(valid) == n
    key_set = {int(k) for k, kp, v in zip(keys, keep, valid) if kp and v}
    has_null = bool(np.any(keep & ~valid))
    return key_set, has_null


def in_set(values, valid, key_set, has_null):
    """x IN SET s for every probe row, as x IN (the set's keys [, NULL]): a NULL row is UNKNOWN; the empty set without a NULL is
    FALSE everywhere, NULL rows included (an OR of nothing); a match is TRUE; a non-match is FALSE, or UNKNOWN when the build
    side held a NULL."""
    values = np.asarray(values, dtype=np.int64)
    n = len(values)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    if not key_set and not has_null:
        return np.zeros(n, bool), np.ones(n, bool)
    keys = np.fromiter(key_set, dtype=np.int64, count=len(key_set))
    match = np.isin(values, keys) & valid
    t = match
    f = np.zeros(n, bool) if has_null else (valid & ~match)
    return t, f


def not_(a):
    return a[1], a[0]


def and_(a, b):
    return a[0] & b[0], a[1] | b[1]


def or_(a, b):
    return a[0] | b[0], a[1] & b[1]


def compare(values, valid, op, literal):
    """An integer comparison leaf, for the predicates the tests put beside a set leaf"""
    values = np.asarray(values, dtype=np.int64)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    r = {"=": values == literal, "!=": values != literal, "<": values < literal, "<=": values <= literal, ">": values > literal, ">=": values >= literal}[op]
    return r & valid, ~r & valid


def kept(a):
    """The rows a filter with this root keeps"""
    return np.flatnonzero(a[0])
