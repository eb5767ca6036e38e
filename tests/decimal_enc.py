"""A byte-exact writer of Decimal128 DATA streams (zigzag LEB128 varints of an i128) and a plain model of the Decimal128 and
Timestamp value decoders.  TEST INFRASTRUCTURE ONLY (the sibling of rle2_enc.py, deflate_enc.py and lzo_enc.py).

WRITERS take what the bytes can say, not what an encoder would pick: a varint padded with continuation bytes that carry no
payload (over-long forms: up to 19 bytes they are valid, beyond that malformed), and a raw form written from its 7-bit groups, so
that the 19th byte can carry bits above bit 127.  Two fillers of KNOWN values bring a case to a chosen stream offset: one of
1-byte varints, one of 8-byte varints (a 64 KiB boundary is then 8192 values away, not 65536).

MODEL: Python integers only, written from the reference's text:

  * decode(): encoding/decimal.rs:38-52 calls read_varint_zigzagged::<i128, _, SignedEncoding> value by value
    (encoding/integer/util.rs:475-498, :522-527, :536-548; oracle: oo_varint128_decode).  A byte is READ (encoding/util.rs:26-30:
    read_exact, IoError at the end of the stream) before its shift amount is looked at; `checked_shl(offset)` of an i128 fails
    from offset 128 on (VarintTooLarge) -- so the 20th byte of a varint is the one that fails, and a stream that ends behind 19
    continuation bytes is an IoError --; below 128 the payload bits that leave the 128 are dropped silently (byte 19 sits at
    offset 126: two of its seven bits stay); zigzag is undone in 128 bits (unsigned_shr).
  * fix_scale(): array_decoder/decimal.rs:138-166 in a release build.  The value's scale is taken `as u32` (a negative one is
    2^32 - |s|); 10_i128.pow(k) wraps modulo 2^128 and is read as signed; `/` truncates toward zero; `*` wraps.  From k = 128 on
    the wrapped power is 0 (2^128 divides 10^128) and the division PANICS: the model says PANICS and invents nothing
    (DESIGN.md section 2 says what oracle and HIP path do there).  Multiplication only happens for k <= the column's scale.
  * decode_timestamp(): encoding/timestamp.rs:121-192.  The SECONDARY value is taken `as u64`; its low three bits z != 0 mean
    "times 10^(z + 1)", a wrapping u64 multiply; seconds + base wraps in i64; seconds below the epoch with more than 999 999
    nanoseconds lose one second (ORC-763) -- the nanoseconds are NOT bounded by 10^9 --; the sum is an i128; a unit that does not
    divide it, or a quotient outside i64, is DecodeTimestamp.  The Decimal128(38, 9) target (timestamp.rs:194-197) is the i128
    sum itself and cannot fail.
"""

IO_ERROR, VARINT_TOO_LARGE, DECODE_TIMESTAMP = 1, 3, 4  # the error kinds, numbered as oracle_lib numbers them
PANICS = "PANICS"
M64, M128 = (1 << 64) - 1, (1 << 128) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
SECONDS, MILLIS, MICROS, NANOS, DECIMAL128 = 0, 1, 2, 3, 4  # the timestamp targets
NANOS_PER_UNIT = (10**9, 10**6, 10**3, 1)


# ---- writers --------------------------------------------------------------------------------------------------------------------
def zigzag(v):
    assert I128_MIN <= v <= I128_MAX
    return ((v << 1) ^ (v >> 127)) & M128


def groups_of(u):
    """the 7-bit groups of u, least significant first, without leading zero groups (zero: one group)"""
    out = [u & 0x7F]
    while u >> 7:
        u >>= 7
        out.append(u & 0x7F)
    return out


def raw(groups):
    """a varint from its 7-bit groups as they are: every byte but the last carries the continuation flag"""
    assert groups and all(0 <= g < 128 for g in groups)
    return bytes([g | 0x80 for g in groups[:-1]] + [groups[-1]])


def varint(value, nbytes=None):
    """zigzag LEB128 of an i128; nbytes: padded to that length with continuation bytes whose payload is zero"""
    g = groups_of(zigzag(value))
    if nbytes is not None:
        assert nbytes >= len(g), (value, nbytes)
        g += [0] * (nbytes - len(g))
    return raw(g)


def fill1(count, at=0):
    """`count` 1-byte varints (values -64 .. 63), the `at`-th and following of an endless pattern: (bytes, values)"""
    us = [((at + i) * 37 + 11) & 0x7F for i in range(count)]
    return bytes(us), [(u >> 1) ^ -(u & 1) for u in us]


def fill8(count, at=0):
    """`count` 8-byte varints (50 - 56 bits of payload, both signs): (bytes, values)"""
    us = [(1 << 55) | (((at + i + 1) * 0x9E3779B97F4A7C15) & ((1 << 55) - 1)) for i in range(count)]
    return b"".join(raw(groups_of(u)) for u in us), [(u >> 1) ^ -(u & 1) for u in us]


def fill_bytes(nbytes, at=0):
    """valid varints of exactly nbytes bytes: 8-byte ones, then 1-byte ones for the rest"""
    b8, v8 = fill8(nbytes // 8, at)
    b1, v1 = fill1(nbytes % 8, at)
    return b8 + b1, v8 + v1


def present_rows(n_values, every=5):
    """a PRESENT pattern of about 20 % nulls that holds n_values non-null rows: every `every`-th row is null, the last row is not"""
    rows, have = [], 0
    while have < n_values:
        rows.append(0 if len(rows) % every == every - 1 else 1)
        have += rows[-1]
    return rows


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _signed(u, nbits):
    u &= (1 << nbits) - 1
    return u - (1 << nbits) if u >> (nbits - 1) else u


def decode(stream, n):
    """The first n values of the stream, or (error kind, index of the failing value, the values in front of it)."""
    stream, pos, vals = bytes(stream), 0, []
    while len(vals) < n:
        num, offset = 0, 0
        while True:
            if pos >= len(stream):
                return IO_ERROR, len(vals), vals
            b = stream[pos]
            pos += 1
            if offset >= 128:
                return VARINT_TOO_LARGE, len(vals), vals
            num = (num | ((b & 0x7F) << offset)) & M128
            offset += 7
            if not b & 0x80:
                break
        vals.append(_signed((num >> 1) ^ -(num & 1), 128))
    return vals


def fix_scale(v, fixed_scale, varying_scale):
    """the value at the column's scale, or PANICS where the reference divides by a wrapped power of ten that is zero"""
    vs = varying_scale & 0xFFFFFFFF
    if fixed_scale == vs:
        return v
    if fixed_scale < vs:
        factor = _signed(pow(10, vs - fixed_scale, 1 << 128), 128)
        if factor == 0:
            return PANICS
        q = abs(v) // abs(factor)
        return _signed(q if (v < 0) == (factor < 0) else -q, 128)
    return _signed(v * _signed(pow(10, fixed_scale - vs, 1 << 128), 128), 128)


def decode_timestamp(base, seconds, nanos, unit):
    """the value in `unit` (DECIMAL128: the i128 nanoseconds), or DECODE_TIMESTAMP"""
    nn = nanos & M64
    zeros = nn & 7
    nn >>= 3
    if zeros:
        nn = (nn * 10 ** (zeros + 1)) & M64
    sse = _signed(seconds + base, 64)
    s = _signed(sse - 1, 64) if sse < 0 and nn > 999_999 else sse
    ns = s * 10**9 + nn
    if unit == DECIMAL128:
        return ns
    per = NANOS_PER_UNIT[unit]
    if ns % per:
        return DECODE_TIMESTAMP
    q = ns // per
    return q if I64_MIN <= q <= I64_MAX else DECODE_TIMESTAMP
