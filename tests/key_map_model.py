"""A plain model of the key maps and lookup columns of include/orcgpu.h ("Key maps and lookup columns"): a dict, and nothing of
the library.

build:  the kept rows of the build side give {key: (value, ...)}; a kept row whose key is NULL sets has_null and holds no values;
        a kept key that comes twice makes the map DUPLICATE (the seal's refusal); a NULL value is stored as None.
probe:  a row's lookup value is the map's value for the row's key -- None where the key is NULL, where the map has no such key,
        and where the stored value is None (LEFT JOIN).
Values are Python ints (Int64; a Decimal128's unscaled integer; a Date's days) and floats; the tests compare floats by their bits."""
import struct

SENTINEL = -0x7F7F7F7F7F7F7F80  # the int64 whose bytes are all 0x80: a free slot while a map is built, and a legal key
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


class Duplicate(Exception):
    """The build saw a kept, non-NULL key twice."""


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def build(keys, rows, kept=None, max_keys=None):
    """keys: per build row the key or None.  rows: per build row the tuple of its values (None: NULL).  kept: per build row
    whether the selection and the filter keep it (None: all).  Returns (map, has_null); raises Duplicate, and OverflowError when
    more than max_keys distinct keys arrive."""
    out, has_null = {}, False
    for i, k in enumerate(keys):
        if kept is not None and not kept[i]:
            continue
        if k is None:
            has_null = True
            continue
        k = int(k)
        if k in out:
            raise Duplicate(k)
        out[k] = tuple(rows[i])
    if max_keys is not None and len(out) > max_keys:
        raise OverflowError(len(out))
    return out, has_null


def probe(m, keys, value):
    """The lookup column of value index `value` for the probe keys (None: a NULL key)."""
    out = []
    for k in keys:
        row = m.get(int(k)) if k is not None else None
        out.append(None if row is None else row[value])
    return out


def why_null(m, key, value):
    """Which of the three ways made a row NULL: "key", "absent", "value"; None: it is not NULL."""
    if key is None:
        return "key"
    if int(key) not in m:
        return "absent"
    return "value" if m[int(key)][value] is None else None
