"""The model of GROUP BY over the kept rows (include/orcgpu.h, orcgpu_result_aggregate_groups), in plain Python: a dict over key
tuples in first-appearance order, the values of every group from the functions of tests/agg_model.py.  A key is what
orc_rust_amd.aggregate.key_of gives: int (Byte .. Long, Date as days, Timestamp in its unit), bool, decimal.Decimal, str (the
exported bytes: a Char value with its padding), or None for the NULL key -- a key value of its own.
TEST INFRASTRUCTURE: nothing here is used by the product."""
import decimal

import numpy as np
import pyarrow as pa

import agg_model as AM

GROUP_MAX, GROUP_KEY_BYTES, GROUP_MAX_KEYS = 256, 64, 4
TOO_MANY, KEY_TOO_LONG = "too many groups", "key too long"      # what the data-dependent refusals are to the model


def key_values(col, ts_unit="ns"):
    """the key of every row in one key column"""
    t = col.type
    if pa.types.is_boolean(t):
        return col.to_pylist()
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return col.to_pylist()
    if pa.types.is_decimal(t):
        return col.to_pylist()          # decimal.Decimal at the column's scale
    if pa.types.is_floating(t) or pa.types.is_binary(t):
        raise TypeError("%s is not a key kind" % t)
    vals, family, _ = AM.column_values_of(col, ts_unit)
    assert family in ("int", "date", "timestamp"), family
    return vals


def key_id(v):
    """what makes two keys of one column the same key: the type beside the value, so that False, 0 and '' stay apart; a Decimal
    by its unscaled digits (one column has one scale)"""
    if isinstance(v, decimal.Decimal):
        return ("dec", v.as_tuple())
    if isinstance(v, int) and not isinstance(v, bool):      # (a Timestamp key is an int with `.units`)
        return ("int", int(v))
    return (type(v).__name__, v)


def group_rows(table, group_by, keep, ts_unit="ns"):
    """[(keys tuple, bool mask of the group's kept rows)] in order of the group's first kept row"""
    cols = [key_values(table.column(k), ts_unit) for k in group_by]
    groups, order = {}, []
    for row in np.flatnonzero(keep):
        keys = tuple(c[row] for c in cols)
        ident = tuple(key_id(k) for k in keys)
        if ident not in groups:
            groups[ident] = (keys, np.zeros(table.num_rows, bool))
            order.append(ident)
        groups[ident][1][row] = True
    return [groups[i] for i in order]


def aggregate_groups(table, specs, group_by, pred=None, selectors=None, batch_size=1024, ts_unit="ns", keep=None):
    """The list orcgpu_result_aggregate_groups / ArrowReaderBuilder.aggregate(group_by=...) give for `table`: [(keys tuple, values
    list)], the values as AM.aggregate gives them; TOO_MANY / KEY_TOO_LONG where the call is refused after its wait."""
    assert 1 <= len(group_by) <= GROUP_MAX_KEYS and len(set(group_by)) == len(group_by)
    if keep is None:
        keep = AM.kept_mask(table, pred, selectors, batch_size)
    groups = group_rows(table, group_by, keep, ts_unit)
    if len(groups) > GROUP_MAX:
        return TOO_MANY
    for keys, _ in groups:
        if any(isinstance(k, str) and len(k.encode()) > GROUP_KEY_BYTES for k in keys):
            return KEY_TOO_LONG
    return [(keys, AM.aggregate(table, specs, keep=mask, ts_unit=ts_unit)) for keys, mask in groups]


def merge_stripes(parts):
    """first-appearance order across stripes: the keys of [[(keys, values)] per stripe] in the order the reader reports them"""
    seen, order = set(), []
    for part in parts:
        for keys, _ in part:
            ident = tuple(key_id(k) for k in keys)
            if ident not in seen:
                seen.add(ident)
                order.append(keys)
    return order
