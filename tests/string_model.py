"""A plain model of the reference's String / Binary column decoders: Python integers and bytes, nothing of the oracle or the
HIP code.

direct()      GenericByteArrayDecoder::next_byte_batch (array_decoder/string.rs:111-153), batch by batch:
                1. the batch's lengths (0 in null rows) are summed as i64, the sum wrapping as the release build's does; a sum above
                   i32::MAX is OffsetOverflow
                2. a negative length is an Arrow error (the offsets cannot be formed)
                3. the next `sum` bytes of DATA are taken; fewer of them is an Arrow error (offsets past the values, try_new)
                4. the offsets restart at 0
                5. Utf8: the batch's bytes are validated on their own, then every offset strictly inside them must not be on a
                   continuation byte (GenericStringType::validate)
dictionary()  DictionaryStringArrayDecoder (string.rs:65-82, :204-224): the dictionary is ONE such batch of dictionary_size entries
              without PRESENT -- a failure there fails the column before any batch --; per batch every non-null key must lie in
              0 .. dictionary_size (DictionaryArray::try_new), the entries are gathered (cast to Utf8), null rows are empty strings,
              a gathered total above i32::MAX is an Arrow error.

UTF-8 is judged by bytes.decode("utf-8"), strict: no surrogates, no overlong forms, nothing above U+10FFFF -- what Rust's
from_utf8 accepts.  Binary is direct(utf8=False); Char and Varchar decode as String."""
OFFSET_OVERFLOW, ARROW = 5, 8  # the error kinds, numbered as oracle_lib numbers them
I32_MAX = (1 << 31) - 1
CONSTRUCTION = -1  # "failing batch" of a dictionary that cannot be built: the column fails before batch 0


def i64(v):
    """a decoded LENGTH / DATA value as the reference holds it: 64 bits, read as signed"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def utf8_ok(data):
    try:
        bytes(data).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def byte_batch(lengths, data, at, utf8):
    """One batch over the spaced lengths: (offsets, values, bytes of DATA consumed) or the error kind."""
    lengths = [i64(v) for v in lengths]
    total = i64(sum(lengths))
    if total > I32_MAX:
        return OFFSET_OVERFLOW
    if any(v < 0 for v in lengths):
        return ARROW
    # (total as u64: a wrapped, negative sum asks for more bytes than any stream has)
    if (total & ((1 << 64) - 1)) > len(data) - at:
        return ARROW
    values = bytes(data[at:at + total])
    offsets = [0]
    for v in lengths:
        offsets.append(offsets[-1] + v)
    if utf8:
        if not utf8_ok(values):
            return ARROW
        if any(o < len(values) and values[o] & 0xC0 == 0x80 for o in offsets):
            return ARROW
    return offsets, values, total


def spaced(dense, rows):
    it = iter(dense)
    return [next(it) if r else 0 for r in rows]


def validity_of(rows):
    """None for a batch without a null row (string.rs:145-149), else one bool per row"""
    return None if all(rows) else [bool(r) for r in rows]


def direct(lengths, present, data, batch, utf8):
    """lengths: the decoded LENGTH values, one per non-null row; present: one 0/1 per row, or None.
    Returns ([(offsets, values, validity)] of the Ok batches, None or (kind, index of the first failing batch))."""
    rows = [1] * len(lengths) if present is None else list(present)
    assert sum(1 for r in rows if r) == len(lengths)
    out, at, di = [], 0, 0
    for b, r0 in enumerate(range(0, len(rows), batch)):
        brows = rows[r0:r0 + batch]
        k = sum(1 for r in brows if r)
        got = byte_batch(spaced(lengths[di:di + k], brows), data, at, utf8)
        di += k
        if not isinstance(got, tuple):
            return out, (got, b)
        out.append((got[0], got[1], None if present is None else validity_of(brows)))
        at += got[2]
    return out, None


def dictionary(dict_lengths, dict_data, dictionary_size, keys, present, batch):
    """keys: the decoded DATA values, one per non-null row.  Returns like direct(); a dictionary that cannot be built is
    ([], (kind, CONSTRUCTION))."""
    assert len(dict_lengths) >= dictionary_size
    built = byte_batch(dict_lengths[:dictionary_size], dict_data, 0, True)
    if not isinstance(built, tuple):
        return [], (built, CONSTRUCTION)
    doff, dbytes, _ = built
    rows = [1] * len(keys) if present is None else list(present)
    assert sum(1 for r in rows if r) == len(keys)
    out, di = [], 0
    for b, r0 in enumerate(range(0, len(rows), batch)):
        brows = rows[r0:r0 + batch]
        k = sum(1 for r in brows if r)
        bkeys = [i64(v) for v in keys[di:di + k]]
        di += k
        if any(not 0 <= v < dictionary_size for v in bkeys):
            return out, (ARROW, b)
        it = iter(bkeys)
        offsets, parts = [0], []
        for r in brows:
            entry = b""
            if r:
                v = next(it)
                entry = dbytes[doff[v]:doff[v + 1]]
            parts.append(entry)
            offsets.append(offsets[-1] + len(entry))
        if offsets[-1] > I32_MAX:
            return out, (ARROW, b)
        out.append((offsets, b"".join(parts), None if present is None else validity_of(brows)))
    return out, None
