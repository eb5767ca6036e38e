"""A bit-exact Zstandard frame writer (RFC 8878) for the tests.  TEST INFRASTRUCTURE ONLY, the sibling of deflate_enc.py.

Nothing here compresses: the caller says which frame header fields, which blocks, which literals form, which Huffman
weights, which table modes and which sequences go into the frame, and the writer keeps a Python model of what a decoder must
produce, so every frame carries its own expected plain bytes.  No FSE encoder is needed: the DECODING table is built as the
RFC specifies and the states are chosen backwards (for a next state and a symbol there is exactly one state of that symbol
whose [baseline, baseline + 2^nbits) holds the next state; the state written first -- the last symbol's -- is free).

    f = Frame(fcs_bytes=1)                        # Single_Segment, 1-byte content size
    f.raw(b"abc")                                 # Raw_Block
    f.rle(0x41, 100)                              # RLE_Block
    f.compressed(RawLit(b"xyz"), [S(3, 5, 2), Rep(0, 4, 1)], ll=PREDEF, of=Rle(), ml=Fse(), last=True)
    payload, plain = f.finish(), f.plain()

Sequences: S(literals_length, match_length, offset) writes the offset itself (offset value = offset + 3, never a repeat code);
Rep(literals_length, match_length, code) asks for repeat-offset code 1, 2 or 3 by name: the writer tracks the repeat history,
the literals_length == 0 shift and its carry across blocks included."""
from collections import namedtuple

from deflate_enc import limited_lengths

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 * 1024

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192,
           16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEFAULT[0]) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEFAULT[0]) == 53 and len(OF_DEFAULT[0]) == 29
LL, OF, ML = 0, 1, 2                       # the order of the modes byte and of the table descriptions
DEFAULTS = [LL_DEFAULT, OF_DEFAULT, ML_DEFAULT]
MAX_LOG = [9, 8, 9]
MAX_SYMBOL = [35, 31, 52]

S = namedtuple("S", "ll ml offset")
Rep = namedtuple("Rep", "ll ml code")


# ---- table modes of the sequences section -------------------------------------------------------------------------------------
class Predefined:
    mode = 0


class Rle:
    """RLE_Mode: the table is one symbol (None: the code of the block's sequences, which must then all share it)."""
    mode = 1

    def __init__(self, symbol=None):
        self.symbol = symbol


class Fse:
    """FSE_Compressed_Mode.  norm: the normalised counts (-1: "less than 1"); None: derived from the block's codes with
    `log` as accuracy log, the rare codes (`low`) given -1."""
    mode = 2

    def __init__(self, norm=None, log=None, low=()):
        self.norm, self.log, self.low = norm, log, low


class Repeat:
    mode = 3


PREDEF = Predefined()
REPEAT = Repeat()


# ---- literals -----------------------------------------------------------------------------------------------------------------
class RawLit:
    """Raw_Literals_Block.  fmt: Size_Format 0 (5 bits; its second bit is the size's lowest), 1 (12 bits) or 3 (20 bits); None: the shortest."""
    def __init__(self, data=b"", fmt=None):
        self.data, self.fmt = bytes(data), fmt


class RleLit:
    def __init__(self, byte, n, fmt=None):
        self.data, self.fmt = bytes([byte]) * n, fmt


class HufLit:
    """Compressed_Literals_Block, or Treeless_Literals_Block (treeless=True: the frame's last tree).  fmt: Size_Format 0 (one
    stream, 10-bit sizes), 1, 2, 3 (four streams; 10, 14, 18 bits); None: 0 for streams == 1, else the shortest of 1..3.
    weights: the tree, one weight per symbol 0..last (the last one is implied in the description and must be what the others
    leave); None: a length-limited Huffman code of the data.  desc: "direct" (4-bit weights), "fse" or None (direct where it fits)."""
    def __init__(self, data, streams=4, fmt=None, weights=None, desc=None, treeless=False, fse_log=6):
        self.data, self.streams, self.fmt, self.weights, self.desc, self.treeless, self.fse_log = bytes(data), streams, fmt, weights, desc, treeless, fse_log


def size_format_bits(fmt):
    return {0: 5, 1: 12, 3: 20}[fmt]


# ---- bits ---------------------------------------------------------------------------------------------------------------------
def backward_stream(reads):
    """The bytes of a stream that is read backwards: `reads` lists (value, nbits) in the order the DECODER reads them.  The
    final-bit marker sits above the first field read; its position in the last byte is whatever the bit count leaves."""
    s = ["1"]
    for v, nb in reads:
        if nb:
            assert 0 <= v < (1 << nb), (v, nb)
            s.append(format(v, "0%db" % nb))
    s = "".join(s)
    return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


class ForwardBits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb), (v, nb)
        self.acc |= v << self.n
        self.n += nb

    def getvalue(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- FSE ----------------------------------------------------------------------------------------------------------------------
class FseTable:
    """The decoding table of RFC 8878 4.1.1 and its inverse: before[symbol][next state] = the one state of that symbol to come from."""
    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
        high, sym, nxt = size - 1, [None] * size, []
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
                nxt.append(1)
            else:
                nxt.append(c)
        step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & mask
                while pos > high:
                    pos = (pos + step) & mask
        assert pos == 0
        self.log, self.norm, self.states = log, list(norm), []
        self.before = {}
        for i in range(size):
            s = sym[i]
            ns = nxt[s]
            nxt[s] += 1
            nb = log - (ns.bit_length() - 1)
            base = (ns << nb) - size
            self.states.append((s, nb, base))
            d = self.before.setdefault(s, {})
            for v in range(base, base + (1 << nb)):
                assert v not in d
                d[v] = i

    @classmethod
    def rle(cls, symbol):
        t = cls.__new__(cls)
        t.log, t.norm, t.states, t.before = 0, None, [(symbol, 0, 0)], {symbol: {0: 0}}
        return t

    def chain(self, symbols, last_state=None, widest=False):
        """The states that emit `symbols` in order.  The last one is free: the given one, else its symbol's lowest state (widest:
        the one with the most bits)."""
        for s in symbols:
            assert s in self.before, ("the table has no state for symbol", s)
        if last_state is None:
            own = [i for i, st in enumerate(self.states) if st[0] == symbols[-1]]
            last_state = max(own, key=lambda i: self.states[i][1]) if widest else own[0]
        assert self.states[last_state][0] == symbols[-1]
        out = [last_state]
        for s in reversed(symbols[:-1]):
            out.append(self.before[s][out[-1]])
        out.reverse()
        return out

    def update(self, state, nxt):
        """(value, nbits) the decoder reads to go from `state` to `nxt`"""
        _, nb, base = self.states[state]
        assert base <= nxt < base + (1 << nb) or (nb == 0 and nxt == base)
        return nxt - base, nb


def fse_description(norm, log):
    """RFC 8878 4.1.1: the accuracy log and the counts, with the zero-run repeat flags; (bytes, bits used)."""
    w = ForwardBits()
    w.put(log - 5, 4)
    remaining, threshold, nbits, i = (1 << log) + 1, 1 << log, log + 1, 0
    while remaining > 1 and i < len(norm):
        c = norm[i]
        i += 1
        v, mx = c + 1, (2 * threshold - 1) - remaining
        if v < mx:
            w.put(v, nbits - 1)
        elif v < threshold:
            w.put(v, nbits)
        else:
            w.put(v + mx, nbits)
        remaining -= abs(c)
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if c == 0:
            run = 0
            while i < len(norm) and norm[i] == 0:
                run += 1
                i += 1
            while run >= 3:
                w.put(3, 2)
                run -= 3
            w.put(run, 2)
    return w.getvalue(), w.n


def normalise(freq, log, low=()):
    """Counts that sum to 2^log, at least 1 for every symbol in use; the symbols of `low` get -1."""
    size = 1 << log
    used = [s for s, f in enumerate(freq) if f]
    norm = [0] * (max(used) + 1)
    for s in low:
        assert freq[s]
        norm[s] = -1
    rest = [s for s in used if s not in low]
    room, total = size - len(low), sum(freq[s] for s in rest)
    assert rest and room >= len(rest), "the accuracy log is too low for that many symbols"
    for s in rest:
        norm[s] = max(1, freq[s] * room // total)
    while sum(abs(c) for c in norm) > size:
        norm[max(rest, key=lambda s: norm[s])] -= 1
    norm[max(rest, key=lambda s: freq[s])] += size - sum(abs(c) for c in norm)
    return norm


# ---- Huffman ------------------------------------------------------------------------------------------------------------------
def huffman_weights(data, limit=11):
    """Weights of a complete code for the bytes of `data`, none longer than `limit` bits (a lone symbol gets a partner)."""
    freq = [0] * 256
    for b in data:
        freq[b] += 1
    if sum(1 for f in freq if f) < 2:
        freq[(data[0] ^ 1) if data else 0] += 1
        if not data:
            freq[1] += 1
    lens = limited_lengths(freq, limit)
    top = max(lens)
    last = max(s for s in range(256) if lens[s])
    return [top + 1 - l if l else 0 for l in lens[:last + 1]]


def huffman_codes(weights):
    """{symbol: (code, nbits)}: the prefix codes RFC 8878 4.2.1.3 gives the weights (ranked by weight, then by symbol)."""
    total = sum(1 << (w - 1) for w in weights if w)
    maxbits = total.bit_length() - 1
    assert total == 1 << maxbits, ("the weights do not sum to a power of two", total)
    codes, pos = {}, 0
    for w in range(1, maxbits + 2):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (pos >> (w - 1), maxbits + 1 - w)
                pos += 1 << (w - 1)
    return codes, maxbits


def huffman_stream(codes, data):
    return backward_stream([codes[b] for b in data])


def weights_direct(listed):
    assert 1 <= len(listed) <= 128
    out = bytearray([127 + len(listed)])
    for i in range(0, len(listed), 2):
        out.append((listed[i] << 4) | (listed[i + 1] if i + 1 < len(listed) else 0))
    return bytes(out)


def weights_fse(listed, log=6, norm=None):
    """The weights as an FSE stream of two interleaved states (RFC 8878 4.2.1.2): the header byte, the table description, the stream."""
    assert len(listed) >= 2
    if norm is None:
        freq = [0] * 13
        for w in listed:
            freq[w] += 1
        norm = normalise(freq, log)
    t = FseTable(norm, log)
    chains = []
    for k in (0, 1):
        mine = listed[k::2]
        # the state that emits the last weight but one must need bits the stream no longer has: that is how the decoder sees the end
        want_bits = (len(listed) - 2) % 2 == k
        own = [i for i, st in enumerate(t.states) if st[0] == mine[-1] and (st[1] > 0 or not want_bits)]
        assert own, "no state that needs bits for the last weight but one"
        chains.append(t.chain(mine, last_state=own[0]))
    reads = [(chains[0][0], log), (chains[1][0], log)]
    for i in range(2, len(listed)):
        c = chains[i % 2]
        reads.append(t.update(c[i // 2 - 1], c[i // 2]))
    desc, _ = fse_description(norm, log)
    body = desc + backward_stream(reads)
    assert len(body) < 128, ("the compressed weights take more than 127 bytes", len(body))
    return bytes([len(body)]) + body


# ---- lengths and offsets ------------------------------------------------------------------------------------------------------
def length_code(base, value):
    c = max(i for i in range(len(base)) if base[i] <= value)
    return c, value - base[c]


class Frame:
    """One Zstandard frame under construction and the plain bytes it must decode to (check=False: a damaged frame; the model then
    only follows what it can).

    fcs_bytes: the width of Frame_Content_Size (1: Single_Segment with the 1-byte form; 2, 4, 8 with single_segment either way;
    0: none, which needs a window descriptor).  fcs: the value written (None: the model's size).  window: the descriptor byte
    (None: 1 MiB where one is needed).  dict_id: (width 1 / 2 / 4, value) or None.  checksum: True, or "wrong"."""

    def __init__(self, fcs_bytes=1, single_segment=None, fcs=None, window=None, dict_id=None, checksum=False, reserved=False, check=True):
        self.fcs_bytes, self.fcs, self.window, self.dict_id, self.checksum, self.reserved, self.check = fcs_bytes, fcs, window, dict_id, checksum, reserved, check
        self.single = (fcs_bytes != 0) if single_segment is None else single_segment
        assert not (self.single and fcs_bytes == 0) and not (fcs_bytes == 1 and not self.single)
        self.body = bytearray()
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.weights = None              # the frame's last Huffman tree
        self.tables = [None, None, None]  # the frame's last LL / OF / ML tables
        self.marks = []                  # (name, offset in the body) of what the last compressed block wrote: where to cut or poke

    # ---- the model ----
    def plain(self):
        return bytes(self.out)

    def _copy(self, length, offset):
        if offset > len(self.out) or offset == 0:
            assert not self.check, ("offset beyond the start of the frame", offset, len(self.out))
            return
        start = len(self.out) - offset
        if offset >= length:
            self.out += self.out[start:start + length]
        else:
            self.out += (bytes(self.out[start:]) * (length // offset + 1))[:length]

    # ---- blocks ----
    def _block(self, btype, size, content, last):
        assert 0 <= size < (1 << 21)
        h = int(last) | (btype << 1) | (size << 3)
        self.block_at = len(self.body)
        self.body += h.to_bytes(3, "little") + content
        return self

    def raw(self, data=b"", last=False, size=None):
        self.out += data
        return self._block(0, len(data) if size is None else size, data, last)

    def rle(self, byte, n, last=False):
        self.out += bytes([byte]) * n
        return self._block(1, n, bytes([byte]), last)

    def reserved_block(self, content=b"", last=False):
        return self._block(3, len(content), content, last)

    def compressed(self, lit, seqs=(), ll=PREDEF, of=PREDEF, ml=PREDEF, last=False, nseq_form=None, size=None, modes_reserved=0,
                   nseq=None, widest=False, tamper=None):
        """A Compressed_Block.  nseq_form: 1, 2 or 3 bytes of Number_of_Sequences (None: the shortest); nseq: the count written
        (None: the true one); size: the Block_Size written (None: the true one); tamper: f(section name, bytes) -> bytes, applied to
        "literals", "tables", "bits" before they are put together (damaged blocks)."""
        tamper = tamper or (lambda name, b: b)
        if isinstance(lit, (bytes, bytearray)):
            lit = RawLit(lit)
        lits = lit.data
        content = bytearray(tamper("literals", self._literals(lit)))
        seqs = list(seqs)
        n = len(seqs) if nseq is None else nseq
        if nseq_form is None:
            nseq_form = 1 if n < 128 else 2 if n < 0x7F00 else 3
        if nseq_form == 1:
            assert n < 128
            content.append(n)
        elif nseq_form == 2:
            assert n < 0x7F00
            content += bytes([128 + (n >> 8), n & 255])
        else:
            assert 0x7F00 <= n < 0x7F00 + 65536
            content += bytes([255]) + (n - 0x7F00).to_bytes(2, "little")
        lp = 0
        if seqs:
            coded = []   # per sequence: the three (code, extra value, extra bits), in table order LL, OF, ML
            for q in seqs:
                if isinstance(q, Rep):
                    assert q.code in (1, 2, 3)
                    value = q.code
                    idx = q.code - 1 + (1 if q.ll == 0 else 0)
                    if idx == 0:
                        offset = self.rep[0]
                    else:
                        offset = self.rep[idx] if idx < 3 else self.rep[0] - 1
                        if idx > 1:
                            self.rep[2] = self.rep[1]
                        self.rep[1] = self.rep[0]
                        self.rep[0] = offset
                else:
                    offset, value = q.offset, q.offset + 3
                    self.rep = [offset, self.rep[0], self.rep[1]]
                oc = value.bit_length() - 1
                lc, lx = length_code(LL_BASE, q.ll)
                mc, mx = length_code(ML_BASE, q.ml)
                coded.append(((lc, lx, LL_BITS[lc]), (oc, value - (1 << oc), oc), (mc, mx, ML_BITS[mc])))
                assert lp + q.ll <= len(lits) or not self.check, "more literal lengths than literals"
                self.out += lits[lp:lp + q.ll]
                lp += q.ll
                self._copy(q.ml, offset)
            modes, desc = 0, bytearray()
            for w, spec in ((LL, ll), (OF, of), (ML, ml)):
                modes |= spec.mode << (6 - 2 * w)
                codes = [c[w][0] for c in coded]
                if spec.mode == 0:
                    self.tables[w] = FseTable(*DEFAULTS[w])
                elif spec.mode == 1:
                    sym = codes[0] if spec.symbol is None else spec.symbol
                    if sym != codes[0]:   # (a damaged block: a symbol the sequences do not have, without extra bits)
                        assert not self.check
                        coded = [c[:w] + ((sym, 0, 0),) + c[w + 1:] for c in coded]
                    desc.append(sym)
                    self.tables[w] = FseTable.rle(sym)
                elif spec.mode == 2:
                    norm, log = spec.norm, spec.log
                    if norm is None:
                        freq = [0] * (max(codes) + 1)
                        for c in codes:
                            freq[c] += 1
                        norm = normalise(freq, log, spec.low)
                    d, spec.desc_bits = fse_description(norm, log)
                    desc += d
                    self.tables[w] = FseTable(norm, log)
                else:
                    assert self.tables[w] is not None or not self.check, "Repeat_Mode without a table in the frame"
                    if self.tables[w] is None:
                        self.tables[w] = FseTable(*DEFAULTS[w])   # (a damaged frame: any table will do, the modes byte is the error)
            content.append(modes | modes_reserved)
            content += tamper("tables", bytes(desc))
            t = self.tables
            chains = [t[w].chain([c[w][0] for c in coded], widest=widest) for w in range(3)]
            reads = [(chains[w][0], t[w].log) for w in (LL, OF, ML)]
            for i, c in enumerate(coded):
                reads += [(c[OF][1], c[OF][2]), (c[ML][1], c[ML][2]), (c[LL][1], c[LL][2])]
                if i + 1 < len(coded):
                    reads += [t[w].update(chains[w][i], chains[w][i + 1]) for w in (LL, ML, OF)]
            self.step_bits = max(sum(nb for _, nb in reads[3 + 6 * i:9 + 6 * i]) for i in range(len(coded)))
            content += tamper("bits", backward_stream(reads))
        self.out += lits[lp:]
        return self._block(2, len(content) if size is None else size, bytes(content), last)

    def _literals(self, lit):
        n = len(lit.data)
        if not isinstance(lit, HufLit):
            fmt = lit.fmt if lit.fmt is not None else (0 if n < 32 else 1 if n < 4096 else 3)
            bits = size_format_bits(fmt)
            assert n < (1 << bits)
            kind = 0 if isinstance(lit, RawLit) else 1
            hdr = (kind | (fmt << 2) | (n << (3 if bits == 5 else 4))).to_bytes({5: 1, 12: 2, 20: 3}[bits], "little")
            return hdr + (lit.data if kind == 0 else lit.data[:1])
        body = bytearray()
        if not lit.treeless:
            weights = list(lit.weights) if lit.weights is not None else huffman_weights(lit.data)
            listed = weights[:-1]   # the last weight is implied
            desc = lit.desc or ("direct" if len(listed) <= 128 else "fse")
            body += weights_direct(listed) if desc == "direct" else weights_fse(listed, lit.fse_log)
            self.weights = weights
        assert self.weights is not None or not self.check, "Treeless literals without a tree in the frame"
        codes, self.huf_maxbits = huffman_codes(self.weights if self.weights is not None else huffman_weights(lit.data))
        self.tree_bytes = len(body)
        if lit.streams == 1:
            body += huffman_stream(codes, lit.data)
        else:
            seg = (n + 3) // 4
            parts = [huffman_stream(codes, lit.data[k * seg:(k + 1) * seg]) for k in range(3)] + [huffman_stream(codes, lit.data[3 * seg:])]
            for p in parts[:3]:
                body += len(p).to_bytes(2, "little")
            for p in parts:
                body += p
        fmt = lit.fmt
        if fmt is None:
            fmt = 0 if lit.streams == 1 else 1 if max(n, len(body)) < 1024 else 2 if max(n, len(body)) < 16384 else 3
        assert (fmt == 0) == (lit.streams == 1)
        bits = {0: 10, 1: 10, 2: 14, 3: 18}[fmt]
        assert n < (1 << bits) and len(body) < (1 << bits), (n, len(body), bits)
        hdr = ((3 if lit.treeless else 2) | (fmt << 2) | (n << 4) | (len(body) << (4 + bits))).to_bytes({10: 3, 14: 4, 18: 5}[bits], "little")
        return hdr + bytes(body)

    # ---- the frame ----
    def header(self):
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[self.fcs_bytes]
        did = {None: 0, 1: 1, 2: 2, 4: 3}[self.dict_id and self.dict_id[0]]
        d = (flag << 6) | (int(self.single) << 5) | (int(self.reserved) << 3) | (int(bool(self.checksum)) << 2) | did
        h = bytearray(MAGIC) + bytes([d])
        if not self.single:
            h.append(0x50 if self.window is None else self.window)   # exponent 10: 1 MiB
        if self.dict_id:
            h += self.dict_id[1].to_bytes(self.dict_id[0], "little")
        size = len(self.out) if self.fcs is None else self.fcs
        if self.fcs_bytes == 2:
            size -= 256
        if self.fcs_bytes:
            h += size.to_bytes(self.fcs_bytes, "little")
        return bytes(h)

    def finish(self):
        tail = b""
        if self.checksum:
            import xxhash
            ck = xxhash.xxh64(bytes(self.out), seed=0).intdigest() & 0xFFFFFFFF
            tail = (ck ^ (0x00010000 if self.checksum == "wrong" else 0)).to_bytes(4, "little")
        return self.header() + bytes(self.body) + tail


def skippable(data=b"", nibble=0):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(data).to_bytes(4, "little") + data
