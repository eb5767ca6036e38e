"""A byte-exact writer of integer RLE v1 runs, byte RLE runs and boolean streams, and a plain decoder model of the three.  TEST
INFRASTRUCTURE ONLY (the sibling of rle2_enc.py).

WRITERS take header fields, not data: whatever the header can say can be written, also the forms no encoder picks (a base varint
padded with 0x80 .. 0x00, literal varints of any length, bits above N in a varint's last group, a continuation bit on any byte,
literal groups of one value between runs, payloads that spell headers).  Nothing is checked beyond what the fields can hold.

MODEL: decode_v1(), decode_bytes() and decode_bools() walk a stream run by run with Python integers.  They are written from the ORC
specification and restate the reference where the reference is more particular (integer/rle_v1.rs:54-68, :90-132 and :143-159,
integer/util.rs:475-527 and :536-546, byte.rs:228-247, boolean.rs:48-54 and :101-113, rle.rs:68-107, encoding/util.rs:24-38):

  * varint: a byte is read first (the end of the stream there: IoError), then rejected as VarintTooLarge if its bit offset 7 * i is
    N bits or more (checked_shl), then its seven bits are shifted in -- what is shifted past the top of N falls off.  So a varint
    has at most (N + 6) / 7 bytes -- 10, 5 and 3 for i64, i32 and i16 --, and the last of them holds 1, 4 and 2 bits that count;
  * zigzag is undone in N bits; an unsigned stream takes the N bits as they are (N is a signed type: 2^63 and more reads negative);
  * RLE v1 run: header 0 .. 127 is count - 3, the next byte the delta as an i8, then the base varint.  Every step is a checked add
    (delta >= 0) or a checked subtract of |delta| (delta < 0) in N; a step that leaves N is OutOfSpec and the run delivers NONE of
    its values (the error passes through decode_batch, rle.rs:81-83);
  * RLE v1 literals: a negative header -h means h varints (0x80: 128, 0xff: 1); any varint that fails makes the whole group fail;
  * byte RLE: header below 0x80 is a run of header + 3 copies of the next byte, any other header 0x100 - header literal bytes
    (read_exact: a group that is cut delivers nothing);
  * boolean: byte RLE underneath, a byte's bits from the most significant one down.  A decoder keeps the bits of a byte it has not
    handed out (`data`, `bits_in_data`) for the next call -- a batch size that is no multiple of 8 goes on inside the byte --;
    the unused bits of the stream's last byte are never looked at, whatever they are, and neither are bytes behind the bits asked
    for: a stream that holds more is no error;
  * the end of the stream: RLE v1 reads a run's first byte with try_read_u8 -- no byte there is OutOfSpec ("not enough values to
    decode") --, every other byte with read_u8 / read_exact: IoError.  Byte RLE (and so boolean) reads the header with read_u8 as
    well: the end of the stream is an IoError wherever it comes.

Nothing here panics in the reference (no index, no unchecked arithmetic on what the stream says): PANICS is kept for the tables'
sake and never returned.
"""

IO_ERROR, OUT_OF_SPEC, VARINT_TOO_LARGE = 1, 2, 3  # the error kinds, numbered as oracle_lib numbers them
PANICS = "PANICS"
M64 = (1 << 64) - 1
V1, BYTE, BOOL = "v1", "byte", "bool"  # the codecs of run_sizes() and of the tables


def max_groups(nbits):
    """bytes a varint of N bits may have"""
    return (nbits + 6) // 7


# ---- writers --------------------------------------------------------------------------------------------------------------------
def zigzag(v):
    return ((v << 1) ^ (v >> 63)) & M64


def raw_varint(groups, cont=None):
    """the 7-bit groups as they are, least significant first; cont: the indices whose continuation bit is set (default: all but
    the last).  Bits above N in the last group, a varint that does not end, one that ends early: whatever is asked."""
    cont = set(range(len(groups) - 1)) if cont is None else set(cont)
    return bytes((g & 0x7F) | (0x80 if i in cont else 0) for i, g in enumerate(groups))


def varint(u, length=None):
    """u in `length` bytes: the minimal form, padded with 0x80 .. 0x00 (length None: minimal)"""
    groups = []
    while True:
        groups.append(u & 0x7F)
        u >>= 7
        if not u:
            break
    if length is not None:
        assert length >= len(groups), (length, len(groups))
        groups += [0] * (length - len(groups))
    return raw_varint(groups)


def _unsigned(v, signed, nbits):
    """(nbits: a negative value of an unsigned stream stands for its N bits)"""
    return (zigzag(v) if signed else v) & ((1 << nbits) - 1)


def v1_run(base, delta, count, signed, base_bytes=None, nbits=64):
    assert 3 <= count <= 130 and -128 <= delta <= 127
    return bytes([count - 3, delta & 0xFF]) + varint(_unsigned(base, signed, nbits), base_bytes)


def v1_literals(values, signed, lengths=None, nbits=64):
    assert 1 <= len(values) <= 128
    lengths = lengths or [None] * len(values)
    return bytes([0x100 - len(values)]) + b"".join(varint(_unsigned(v, signed, nbits), n) for v, n in zip(values, lengths))


def byte_run(value, count):
    assert 3 <= count <= 130
    return bytes([count - 3, value & 0xFF])


def byte_literals(values):
    assert 1 <= len(values) <= 128
    return bytes([0x100 - len(values)]) + bytes(v & 0xFF for v in values)


def bool_bytes(bits):
    """the bits packed most significant first, the last byte padded with zeros (the bytes, not yet byte RLE)"""
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


# ---- the model ------------------------------------------------------------------------------------------------------------------
class _Fail(Exception):
    def __init__(self, kind):
        self.kind = kind


class _Input:
    def __init__(self, data):
        self.data, self.pos = bytes(data), 0

    def u8(self):
        if self.pos >= len(self.data):
            raise _Fail(IO_ERROR)
        self.pos += 1
        return self.data[self.pos - 1]

    def take(self, n):
        if self.pos + n > len(self.data):
            self.pos = len(self.data)
            raise _Fail(IO_ERROR)
        self.pos += n
        return self.data[self.pos - n:self.pos]


def _wrap(v, nbits):
    """the low nbits of v, read as a signed number"""
    v &= (1 << nbits) - 1
    return v - (1 << nbits) if v >> (nbits - 1) else v


def _varint(inp, signed, nbits):
    num, shift = 0, 0
    while True:
        b = inp.u8()
        if shift >= nbits:
            raise _Fail(VARINT_TOO_LARGE)
        num |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    num &= (1 << nbits) - 1
    return _wrap((num >> 1) ^ -(num & 1), nbits) if signed else _wrap(num, nbits)


def _v1_run(inp, h, signed, nbits):
    """(rle_v1.rs:60-63: the delta byte is read with the header, in front of the base)"""
    delta = _wrap(inp.u8(), 8)
    vals = [_varint(inp, signed, nbits)]
    for _ in range(h + 2):
        v = vals[-1] + delta  # (subtracting |delta| for a negative one is the same number)
        if _wrap(v, nbits) != v:
            raise _Fail(OUT_OF_SPEC)
        vals.append(v)
    return vals


def _v1_literals(inp, h, signed, nbits):
    return [_varint(inp, signed, nbits) for _ in range(0x100 - h)]


def _byte_group(inp, h):
    if h < 0x80:
        return [_wrap(inp.u8(), 8)] * (h + 3)
    return [_wrap(b, 8) for b in inp.take(0x100 - h)]


def _decode(stream, n_values, eof_kind, group):
    inp, vals, run = _Input(stream), [], 0
    while len(vals) < n_values:
        if inp.pos >= len(inp.data):
            return eof_kind, run, vals
        try:
            vals += group(inp, inp.u8())
        except _Fail as f:
            return f.kind, run, vals
        run += 1
    return vals[:n_values]


def decode_v1(stream, n_values, signed, nbits=64):
    """The first n_values values of the stream, or (error kind, index of the failing run, the values before it)."""
    return _decode(stream, n_values, OUT_OF_SPEC, lambda inp, h: (_v1_run if h < 0x80 else _v1_literals)(inp, h, signed, nbits))


def decode_bytes(stream, n):
    """The first n bytes (as i8, the reference's value type), or (error kind, index of the failing run, the bytes before it)."""
    return _decode(stream, n, IO_ERROR, _byte_group)


def decode_bools(stream, n_bits):
    """The first n_bits bits (0 / 1), or (error kind, index of the failing run, the bits of the bytes before it)."""
    got = decode_bytes(stream, (n_bits + 7) // 8)
    fails = isinstance(got, tuple)
    bits = [(b >> (7 - k)) & 1 for b in (got[2] if fails else got) for k in range(8)]
    return (got[0], got[1], bits) if fails else bits[:n_bits]


def run_sizes(stream, codec):
    """(offset, bytes, values) of every run of a VALID stream, from the headers and the varints' lengths alone (BOOL: counted in
    bytes, as BYTE)"""
    inp, out = _Input(stream), []
    while inp.pos < len(inp.data):
        p = inp.pos
        h = inp.u8()
        n = h + 3 if h < 0x80 else 0x100 - h
        if codec == V1:
            inp.take(1 if h < 0x80 else 0)
            for _ in range(1 if h < 0x80 else n):
                while inp.u8() & 0x80:
                    pass
        else:
            inp.take(1 if h < 0x80 else n)
        out.append((p, inp.pos - p, n))
    return out
