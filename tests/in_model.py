"""The model of the row filter's IN leaf (include/orcgpu.h, ORCGPU_PRED_IN): x IN (v1 .. vk) is OR(x = v1, ..., x = vk) under
three-valued logic, and that is all there is -- `in_leaf` folds or3 over the model's own EQ leaves (tests/filter_model.py, with
tests/filter_model_typed.py for Decimal and Timestamp columns).  `in_leaf_by_set` answers the same question for lists too long to
fold row by row in Python: the literals as a Python set of exact values; tests/test_in_model.py holds it to `in_leaf` on every
corner.  Also here: the probe of the hash set written down in orc_rust_amd/csrc/device/filter_program.h, in plain Python.
TEST INFRASTRUCTURE: nothing here is used by the product."""
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa

import filter_model as FM
import filter_model_typed as FMT
from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P


def literals(pred):
    return [c.value for c in pred.children]


def in_leaf(pred, table):
    """(t, f) of an IN leaf, by definition: the OR of the EQ leaves"""
    n = table.num_rows
    acc = (np.zeros(n, bool), np.ones(n, bool))
    for v in literals(pred):
        acc = FM.or3(acc, FMT.evaluate(P.eq(pred.column, v), table))
    return acc


def in_leaf_by_set(pred, table):
    """(t, f) of an IN leaf through a set of exact keys: ints, floats (no NaN; -0.0 == 0.0 hash alike), bools, bytes, Fractions
    for Decimal, nanoseconds for Timestamp.  The type table is the EQ leaf's: one EQ per literal kind on no rows raises what it raises."""
    vals = literals(pred)
    n = table.num_rows
    if not vals:
        return np.zeros(n, bool), np.ones(n, bool)
    empty = table.slice(0, 0)
    for kind in sorted({v.kind for v in vals}):
        FMT.evaluate(P.eq(pred.column, next(v for v in vals if v.kind == kind)), empty)
    col = table.column(pred.column)
    has_null = any(v.value is None for v in vals)
    keys = set()
    for v in vals:
        x = v.value
        if x is None:
            continue
        if v.kind == PR.PV_FLOAT32:
            x = float(np.float32(x))
        elif v.kind == PR.PV_FLOAT64:
            x = float(x)
        elif v.kind == PR.PV_UTF8:
            x = x.encode() if isinstance(x, str) else bytes(x)
        elif v.kind == PR.PV_DECIMAL128:
            x = Fraction(x[0], 10 ** x[1])
        elif v.kind == PR.PV_BOOLEAN:
            x = bool(x)
        if isinstance(x, float) and x != x:
            continue
        keys.add(x)
    if pa.types.is_decimal(col.type):
        rows = [None if r is None else Fraction(r) for r in col.to_pylist()]
    elif pa.types.is_timestamp(col.type):
        per = FMT.NS_PER_UNIT[col.type.unit]
        rows = [None if r is None else r * per for r in col.cast(pa.int64()).to_pylist()]
    else:
        rows, _ = FM._column_values(col)
    valid = np.array([r is not None for r in rows], bool).reshape(n)
    match = np.array([r is not None and r == r and r in keys for r in rows], bool).reshape(n)
    return valid & match, (np.zeros(n, bool) if has_null else valid & ~match)


def evaluate(pred, table, leaf=in_leaf, other=FMT.evaluate):
    """-> (t, f) over the table's rows: IN leaves by `leaf`, AND / OR / NOT here, every other leaf by `other`"""
    n = table.num_rows
    if pred.op == PR.IN:
        if pred.column not in table.column_names:
            raise FM.FilterRefused(101, "column %r is not there" % pred.column)
        return leaf(pred, table)
    if pred.op == PR.AND:
        acc = (np.ones(n, bool), np.zeros(n, bool))
        for c in pred.children:
            acc = FM.and3(acc, evaluate(c, table, leaf, other))
        return acc
    if pred.op == PR.OR:
        acc = (np.zeros(n, bool), np.ones(n, bool))
        for c in pred.children:
            acc = FM.or3(acc, evaluate(c, table, leaf, other))
        return acc
    if pred.op == PR.NOT:
        return FM.not3(evaluate(pred.children[0], table, leaf, other))
    return other(pred, table)


def or_of_eq(pred):
    """the predicate with every IN leaf spelled as the OR of its EQ leaves: what a caller had to write before"""
    if pred.op == PR.IN:
        return P.or_([P.eq(pred.column, v) for v in literals(pred)])
    if pred.op in (PR.AND, PR.OR, PR.NOT):
        return P(pred.op, children=[or_of_eq(c) for c in pred.children])
    return pred


# ---- the hash set of device/filter_program.h, probed as the kernel probes it ----
M64 = (1 << 64) - 1
IN_KEY_I64, IN_KEY_DEC128, IN_KEY_STRING = 0, 1, 2
HEADER_BYTES = 32


def mix64(k):
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & M64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & M64
    k ^= k >> 33
    return k


def hash_i64(key):
    return mix64(key & M64) & 0xffffffff


def hash_dec128(lo, hi):
    return mix64(lo ^ mix64(hi)) & 0xffffffff


def hash_bytes(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xffffffff
    h ^= h >> 16
    h = h * 0x85ebca6b & 0xffffffff
    h ^= h >> 13
    h = h * 0xc2b2ae35 & 0xffffffff
    h ^= h >> 16
    return h


def float_key(v):
    """a float column's key: the double's bits, -0.0 as 0.0"""
    return struct.unpack("<Q", struct.pack("<d", 0.0 if v == 0 else v))[0]


class Table:
    """A table's bytes taken apart; every part is checked to lie inside them."""

    def __init__(self, blob):
        self.blob = blob
        assert len(blob) >= HEADER_BYTES and len(blob) % 8 == 0
        self.kind, self.n_slots, self.n_keys, self.min_len, self.max_len, self.flags, z0, z1 = struct.unpack_from("<8I", blob, 0)
        assert z0 == 0 and z1 == 0 and self.kind <= IN_KEY_STRING
        assert self.n_slots >= 4 and self.n_slots & (self.n_slots - 1) == 0 and self.n_slots >= 2 * self.n_keys
        occ_words = (self.n_slots + 63) // 64
        self.o_slots = HEADER_BYTES + 8 * occ_words
        self.slot_bytes = 8 if self.kind == IN_KEY_I64 else 16
        self.o_bytes = self.o_slots + self.n_slots * self.slot_bytes
        assert self.o_bytes <= len(blob)
        self.occ = int.from_bytes(blob[HEADER_BYTES:self.o_slots], "little")
        assert bin(self.occ).count("1") == self.n_keys and self.occ >> self.n_slots == 0

    def occupied(self, s):
        return (self.occ >> s) & 1

    def slot(self, s):
        at = self.o_slots + s * self.slot_bytes
        if self.kind == IN_KEY_I64:
            return struct.unpack_from("<Q", self.blob, at)[0]
        if self.kind == IN_KEY_DEC128:
            return struct.unpack_from("<QQ", self.blob, at)
        h, n, off, zero = struct.unpack_from("<4I", self.blob, at)
        assert zero == 0 and self.o_bytes <= off and off + n <= len(self.blob)
        return h, self.blob[off:off + n]

    def probe(self, key):
        """key: an int (two's complement of an int64 taken here), a (low, high) pair of a Decimal, or bytes.  -> (found, steps)"""
        if self.kind == IN_KEY_I64:
            key &= M64
            h = hash_i64(key)
        elif self.kind == IN_KEY_DEC128:
            h = hash_dec128(*key)
        else:
            if not self.min_len <= len(key) <= self.max_len:
                return False, 0
            h = hash_bytes(key)
            key = (h, key)
        s = h & (self.n_slots - 1)
        for step in range(self.n_slots):
            if not self.occupied(s):
                return False, step + 1
            if self.slot(s) == key:
                return True, step + 1
            s = (s + 1) & (self.n_slots - 1)
        return False, self.n_slots

    def keys(self):
        return [self.slot(s) if self.kind != IN_KEY_STRING else self.slot(s)[1] for s in range(self.n_slots) if self.occupied(s)]


def dec128_key(unscaled):
    """(low, high) words of an int128"""
    u = unscaled & ((1 << 128) - 1)
    return u & M64, u >> 64
