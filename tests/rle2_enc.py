"""A bit-exact writer of integer RLE v2 runs and a plain decoder model.  TEST INFRASTRUCTURE ONLY (the sibling of
deflate_enc.py and lzo_enc.py).

WRITERS take header fields, not data: whatever the header can say can be written, also the forms no encoder picks (a width
nobody's percentiles give, gap-255 filler entries the data does not need, a DELTA run of one value, a payload that spells run
headers).  Nothing is checked beyond what the bit fields can hold.

MODEL: decode() walks a stream run by run with Python integers.  It is written from the ORC specification (Integer Run Length
Encoding, version 2) and restates the reference where the reference is more particular than the specification
(rle_v2/mod.rs:112-146, short_repeat.rs:29-63, direct.rs:39-65, patched_base.rs:38-151, delta.rs:44-116, util.rs:44-218 and
:475-569, integer/mod.rs:154-175 and :236-317):

  * the target integer N is i16, i32 or i64 (SHORT; INT and DATE; LONG and the unsigned streams): packed values, SHORT_REPEAT
    values and the DELTA base are N wide (bits above N fall off, zigzag is undone in N bits), the PATCHED_BASE base, the patch
    list and the DELTA deltas are always 64 bits wide;
  * SHORT_REPEAT wider than N bytes, DIRECT wider than N bits: OutOfSpec, before another byte is read;
  * PATCHED_BASE: patch width + gap width above 64 is OutOfSpec; a patch entry is get_closest_fixed_bits(patch width + gap
    width) bits wide -- not the sum --, and the gap is EVERYTHING above the patch bits of the entry, spare bits included; the
    base is sign-magnitude (signed streams; unsigned ones take its bytes as they are), cut to N; a patched slot is
    (value | patch << width) WRAPPING-added to the base in N, every other slot CHECKED-added (OutOfSpec); a patch for a width of
    64 cannot be shifted (OutOfSpec when a patch is due, not before); an entry whose index lies behind the run is never due;
  * DELTA: the first delta is a signed 64-bit varint; > 0 adds, <= 0 SUBTRACTS the magnitudes that follow (so with a zero
    first delta the packed deltas are subtracted; Apache's readers add them); every step is a checked 64-bit operation whose
    result must fit N (OutOfSpec); width code 0 is the fixed delta, width code 1 reads as 2 bits;
  * a varint byte at a shift of N bits or more: VarintTooLarge; bits above N of an earlier byte fall off;
  * the stream ending where a run's first byte is wanted: OutOfSpec; anywhere inside a run: IoError.

Where the reference PANICS the model says PANICS and invents nothing (DESIGN.md section 2 says what oracle and HIP path report
there): an empty patch list (`patches[0]`), a gap-255 filler chain that runs off the list, a packed DELTA run of length 1
(`length - 2`), a first delta of i64::MIN (`abs()`), and PATCHED_BASE packed values wider than N (read_big_endian's slice for
whole bytes, unrolled_unpack_unaligned's assertion otherwise).  `1 << patch_bit_width` with a patch width of 64 -- the fifth
panic the reference's text suggests -- cannot be reached: a patch width of 64 plus a gap width of at least 1 fails the
"greater than 64" test first, so the model reports OutOfSpec there.
"""

WIDTHS = list(range(1, 25)) + [26, 28, 30, 32, 40, 48, 56, 64]  # width code -> bits
IO_ERROR, OUT_OF_SPEC, VARINT_TOO_LARGE = 1, 2, 3  # the error kinds, numbered as oracle_lib numbers them
PANICS = "PANICS"
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def closest_fixed_bits(n):
    """the smallest width the 5-bit code can name that holds n bits (0 -> 1)"""
    return next(w for w in WIDTHS if w >= max(n, 1))


# ---- writers --------------------------------------------------------------------------------------------------------------------
def zigzag(v):
    return ((v << 1) ^ (v >> 63)) & M64


def varint(u):
    out = bytearray()
    while True:
        if u >> 7:
            out.append((u & 0x7F) | 0x80)
            u >>= 7
        else:
            out.append(u)
            return bytes(out)


def pack(values, width):
    """values (their low `width` bits), most significant bit first, back to back; the last byte padded with zeros"""
    acc = 0
    for v in values:
        acc = (acc << width) | (v & ((1 << width) - 1))
    nbits = len(values) * width
    pad = -nbits % 8
    return (acc << pad).to_bytes((nbits + pad) // 8, "big")


def _len_header(kind, width_code, length):
    assert 0 <= width_code < 32 and 1 <= length <= 512
    return bytes([kind << 6 | width_code << 1 | (length - 1) >> 8, (length - 1) & 0xFF])


def short_repeat(value, count, width_bytes, signed):
    assert 3 <= count <= 10 and 1 <= width_bytes <= 8
    u = zigzag(value) if signed else value & M64
    return bytes([(width_bytes - 1) << 3 | (count - 3)]) + (u & ((1 << 8 * width_bytes) - 1)).to_bytes(width_bytes, "big")


def direct(values, width_code, signed):
    return _len_header(1, width_code, len(values)) + pack([zigzag(v) if signed else v for v in values], WIDTHS[width_code])


def msb_base(base, base_bytes, signed):
    """sign-magnitude for a signed stream (a negative zero can be asked for with base = '-0'); an unsigned one: the bytes"""
    if not signed:
        return (base & ((1 << 8 * base_bytes) - 1)).to_bytes(base_bytes, "big")
    neg = base == "-0" or base < 0
    mag = 0 if base == "-0" else abs(base)
    assert mag < 1 << (8 * base_bytes - 1)
    return (mag | (neg << (8 * base_bytes - 1))).to_bytes(base_bytes, "big")


def patched_base(reduced_values, width_code, base, base_bytes, patch_width_code, gap_bits, entries, signed=True, raw_entries=False):
    """entries: (gap, patch) pairs, an entry = gap << patch width | patch; raw_entries: the entries as whole numbers"""
    assert 1 <= base_bytes <= 8 and 1 <= gap_bits <= 8 and len(entries) < 32
    pw = WIDTHS[patch_width_code]
    ew = closest_fixed_bits(min(pw + gap_bits, 64))
    words = list(entries) if raw_entries else [(g << pw) | p for g, p in entries]
    return (_len_header(2, width_code, len(reduced_values)) + bytes([(base_bytes - 1) << 5 | patch_width_code, (gap_bits - 1) << 5 | len(entries)])
            + msb_base(base, base_bytes, signed) + pack(reduced_values, WIDTHS[width_code]) + pack(words, ew))


def delta(base, first_delta, width_code, packed_deltas, length, signed):
    """width code 0: the fixed delta (nothing packed); packed_deltas: the magnitudes of the steps from the third value on"""
    width = WIDTHS[width_code] if width_code else 0
    return (_len_header(3, width_code, length) + varint(zigzag(base) if signed else base & M64) + varint(zigzag(first_delta))
            + (pack(packed_deltas, width) if width else b""))


# ---- the model ------------------------------------------------------------------------------------------------------------------
class _Fail(Exception):
    def __init__(self, kind):
        self.kind = kind


class _Input:
    def __init__(self, data):
        self.data, self.pos = bytes(data), 0

    def take(self, n):
        if self.pos + n > len(self.data):
            self.pos = len(self.data)
            raise _Fail(IO_ERROR)
        self.pos += n
        return self.data[self.pos - n:self.pos]

    def u8(self):
        return self.take(1)[0]


def _wrap(v, nbits):
    """the low nbits of v, read as a signed number"""
    v &= (1 << nbits) - 1
    return v - (1 << nbits) if v >> (nbits - 1) else v


def _unzigzag(v, nbits):
    u = v & ((1 << nbits) - 1)
    return _wrap((u >> 1) ^ -(u & 1), nbits)


def _checked(v, nbits):
    """a 64-bit checked operation whose result must fit N"""
    if not I64_MIN <= v <= I64_MAX or _wrap(v, nbits) != v:
        raise _Fail(OUT_OF_SPEC)
    return v


def _big_endian(inp, n_bytes, nbits):
    if n_bytes * 8 > nbits:
        raise _Fail(PANICS)
    return _wrap(int.from_bytes(inp.take(n_bytes), "big"), nbits)


def _packed(inp, n, width, nbits):
    if width > nbits:
        raise _Fail(PANICS)
    raw = int.from_bytes(inp.take((n * width + 7) // 8), "big") >> (-(n * width) % 8)
    return [_wrap((raw >> (width * (n - 1 - i))) & ((1 << width) - 1), nbits) for i in range(n)]


def _varint(inp, nbits):
    num, shift = 0, 0
    while True:
        b = inp.u8()
        if shift >= nbits:
            raise _Fail(VARINT_TOO_LARGE)
        num |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return _wrap(num, nbits)


def _run_length(h0, h1):
    return ((h0 & 1) << 8 | h1) + 1


def _short_repeat(inp, h, signed, nbits):
    n_bytes = ((h >> 3) & 7) + 1
    if n_bytes * 8 > nbits:
        raise _Fail(OUT_OF_SPEC)
    v = _big_endian(inp, n_bytes, nbits)
    return [_unzigzag(v, nbits) if signed else v] * ((h & 7) + 3)


def _direct(inp, h, signed, nbits):
    width = WIDTHS[(h >> 1) & 31]
    if width > nbits:
        raise _Fail(OUT_OF_SPEC)
    vals = _packed(inp, _run_length(h, inp.u8()), width, nbits)
    return [_unzigzag(v, nbits) for v in vals] if signed else vals


def _patched_base(inp, h, signed, nbits):
    width = WIDTHS[(h >> 1) & 31]
    n = _run_length(h, inp.u8())
    b2, b3 = inp.u8(), inp.u8()
    base_bytes, pw, gw, n_entries = (b2 >> 5) + 1, WIDTHS[b2 & 31], (b3 >> 5) + 1, b3 & 31
    if pw + gw > 64:
        raise _Fail(OUT_OF_SPEC)
    base = int.from_bytes(inp.take(base_bytes), "big")
    if signed:
        sign = 1 << (8 * base_bytes - 1)
        base = -(base & ~sign) if base & sign else base
    base = _wrap(base, nbits)
    vals = _packed(inp, n, width, nbits)
    entries = [v & M64 for v in _packed(inp, n_entries, closest_fixed_bits(pw + gw), 64)]
    at = [0]  # the entry in hand

    def next_patch():
        """(slots to go, patch bits) of the entry in hand, the gap-255 fillers in front of it added up"""
        gap = 0
        while True:
            if at[0] >= len(entries):
                raise _Fail(PANICS)
            g, p = entries[at[0]] >> pw, entries[at[0]] & ((1 << pw) - 1)
            if g != 255 or p != 0:
                return gap + g, p
            gap += 255
            at[0] += 1

    due, patch = next_patch()
    for i in range(n):
        if i == due:
            if width >= 64:
                raise _Fail(OUT_OF_SPEC)
            vals[i] = _wrap((vals[i] | _wrap(patch << width, nbits)) + base, nbits)
            at[0] += 1
            if at[0] < len(entries):
                due, patch = next_patch()
                due += i
        else:
            v = vals[i] + base
            if _wrap(v, nbits) != v:
                raise _Fail(OUT_OF_SPEC)
            vals[i] = v
    return vals


def _delta(inp, h, signed, nbits):
    code = (h >> 1) & 31
    n = _run_length(h, inp.u8())
    base = _varint(inp, nbits)
    if signed:
        base = _unzigzag(base, nbits)
    step = _unzigzag(_varint(inp, 64), 64)
    sign = 1 if step > 0 else -1
    if step == I64_MIN:
        raise _Fail(PANICS)
    step = abs(step)
    vals = [base]
    if code == 0:
        for _ in range(1, n):
            vals.append(_checked(vals[-1] + sign * step, nbits))
        return vals
    vals.append(_checked(base + sign * step, nbits))
    if n < 2:
        raise _Fail(PANICS)
    for d in _packed(inp, n - 2, WIDTHS[code], 64):
        vals.append(_checked(vals[-1] + sign * d, nbits))
    return vals


_KINDS = [_short_repeat, _direct, _patched_base, _delta]


def decode(stream, n_values, signed, nbits=64):
    """The first n_values values of the stream, or (error kind or PANICS, index of the failing run, the values before it)."""
    inp, vals, run = _Input(stream), [], 0
    while len(vals) < n_values:
        if inp.pos >= len(inp.data):
            return OUT_OF_SPEC, run, vals
        try:
            h = inp.u8()
            vals += _KINDS[h >> 6](inp, h, signed, nbits)
        except _Fail as f:
            return f.kind, run, vals
        run += 1
    return vals[:n_values]


def run_sizes(stream):
    """(offset, bytes, values) of every run of a VALID 64-bit stream (the placement helpers of the GPU tests cut streams with it)"""
    inp, out = _Input(stream), []
    while inp.pos < len(inp.data):
        p = inp.pos
        h = inp.u8()
        n = len(_KINDS[h >> 6](inp, h, True, 64))
        out.append((p, inp.pos - p, n))
    return out
