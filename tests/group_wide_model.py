"""The model of the wide GROUP BY path's reduction ("the fold rule"), in numpy float64, written from that text:

    Let r_0 < r_1 < ... < r_(c-1) be the kept input rows of a group.  Lane l (0 .. 63) starts from the empty accumulator (+0.0)
    and folds rows r_l, r_(l+64), r_(l+128), ... into it in that order (acc = acc + value; a NULL value adds nothing); a lane
    l >= c keeps the empty accumulator.  Then, for o = 32, 16, 8, 4, 2, 1, lane l < o takes acc[l] = acc[l] + acc[l + o].
    Lane 0 holds the sum.

and of the numbering of the groups: group g is the g-th distinct key in order of its first kept input row.
TEST INFRASTRUCTURE: nothing here is used by the product, and nothing here calls it."""
import numpy as np

LANES = 64
# the kept-row counts of a group at which the rule changes what it does: one lane; the tree's first partner (lane 1) and its
# last (lanes 31 | 32 | 33 | 63); every lane one row (64); lane 0's second row, the first serial addition (65); a full second
# round and lane 0's third row (128, 129)
THRESHOLD_COUNTS = (1, 2, 32, 33, 63, 64, 65, 128, 129)


def fold_f64(values):
    """The Double SUM of one group: `values` are the column's values of the group's kept rows in ascending input-row order,
    None for NULL.  Returns (sum as np.float64, values that were not NULL)."""
    acc = np.zeros(LANES, np.float64)
    count = 0
    for i, v in enumerate(values):
        if v is None:
            continue
        acc[i % LANES] = acc[i % LANES] + np.float64(v)
        count += 1
    o = LANES // 2
    while o:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[0], count


def group_numbers(keys, keep):
    """keys: an int array, one per input row; keep: bool.  -> (the distinct keys of the kept rows in first-appearance order,
    per input row its group's number or -1)"""
    rows = np.flatnonzero(keep)
    uniq, first, inverse = np.unique(keys[rows], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    numbers = np.full(len(keys), -1, np.int64)
    numbers[rows] = rank[inverse]
    return uniq[order], numbers
