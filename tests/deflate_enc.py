"""A bit-exact raw DEFLATE writer (RFC 1951) for the tests.  TEST INFRASTRUCTURE ONLY, the sibling of lzo_enc.py.

Nothing here compresses: the caller says which blocks, which code lengths and which tokens go into the stream, and the
writer keeps a Python model of what a decoder must produce, so every stream carries its own expected plain bytes.  That
is what real encoders cannot give a test: fixed blocks, stored blocks inside a chunk, 15-bit codes, distance 32768, the
two spellings of length 258, headers at a chosen bit offset, and every kind of damage.

    d = Deflate()
    d.stored(b"abc")                                   # BTYPE 00
    d.fixed([0x41, M(258, 1), M(258, 1, lsym=284)])    # BTYPE 01; the end-of-block code is appended
    d.dynamic(tokens, ll_lens, d_lens, final=True)     # BTYPE 10 from explicit code lengths
    stream, plain = d.finish(), d.plain()

Tokens: an int is a literal byte; M(length, distance[, lsym]) a match; EOB the end-of-block code; RawLL(sym) a bare
literal/length symbol (286, 287: no such length); RawDist(length, dsym) a length followed by a bare distance symbol
(30, 31: no such distance)."""
import heapq
from collections import namedtuple

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 288 symbols: 286 and 287 have codes and no meaning
FIXED_D = [5] * 32                                       # 30 and 31 likewise


class M(namedtuple("M", "length dist lsym")):
    """A match.  lsym: the length symbol to write it with (None: the usual one); 258 may go as 285 or as 284 + extra bits 31."""
    def __new__(cls, length, dist, lsym=None):
        return super().__new__(cls, length, dist, lsym)


RawLL = namedtuple("RawLL", "sym")
RawDist = namedtuple("RawDist", "length dsym")
EOB = "EOB"


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length, the usual way: 258 is symbol 285."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LBASE[i] <= length)
    return 257 + s, LEXT[s], length - LBASE[s]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, DEXT[s], dist - DBASE[s]


def canonical(lens):
    """RFC 1951 3.2.2: the codes of the symbols with a non-zero length (None for the others)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """Sum of 2^-len over the used symbols, in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - l) for l in lens if l)


def limited_lengths(freq, limit):
    """Huffman code lengths for the symbols with freq > 0, none longer than `limit` (flatten the counts until it fits).
    One used symbol gets length 1: an incomplete code, which RFC 1951 allows for a single distance code."""
    used = [i for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    f = {i: freq[i] for i in used}
    while used:
        heap = [(f[i], i, (i,)) for i in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            for s, dd in depth.items():
                lens[s] = dd
            break
        f = {i: (v + 1) // 2 for i, v in f.items()}
    return lens


def split_lengths(n):
    """n code lengths of a COMPLETE code that is as lopsided as 15 bits allow: start from 1, 2, .., 14, 15, 15 and split
    the longest code shorter than 15 bits in two until there are n.  Sorted, shortest first."""
    assert 16 <= n <= 286
    lens = list(range(1, 15)) + [15, 15]
    while len(lens) < n:
        k = max(l for l in lens if l < 15)
        lens.remove(k)
        lens += [k + 1, k + 1]
    return sorted(lens)


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)."""
        assert 0 <= value < (1 << count) or count == 0
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: packed starting with its most significant bit."""
        code &= (1 << length) - 1   # (an over-subscribed code runs out of codes: any bits will do, the header is the error)
        rev = int(format(code, "0%db" % length)[::-1], 2)
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def rle_code_lengths(lens):
    """The usual greedy run-length form of a code length list: [(symbol 0..18, extra value)]."""
    out, i = [], 0
    while i < len(lens):
        v = lens[i]
        run = 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
    return out


class Deflate:
    """A raw DEFLATE stream under construction and the plain bytes it must decode to (`check=False`: a damaged stream; the
    model then only follows what it can)."""

    def __init__(self, check=True):
        self.w = BitWriter()
        self.out = bytearray()
        self.check = check

    # ---- the model ----
    def _copy(self, length, dist):
        if dist > len(self.out):
            assert not self.check, ("distance beyond the start of the output", dist, len(self.out))
            return
        start = len(self.out) - dist
        if dist >= length:
            self.out += self.out[start:start + length]
        else:
            seg = bytes(self.out[start:])
            self.out += (seg * (length // dist + 1))[:length]

    def plain(self):
        return bytes(self.out)

    @property
    def bitpos(self):
        return self.w.bitpos

    # ---- blocks ----
    def stored(self, data=b"", final=False, nlen=None):
        """BTYPE 00.  nlen: the value written as NLEN (None: the one's complement of LEN, as it must be)."""
        assert len(data) <= 65535
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.w.raw(data)
        self.out += data
        return self

    def reserved(self, final=False):
        """BTYPE 11: an error."""
        self.w.bits(int(final), 1)
        self.w.bits(3, 2)
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        self._tokens(tokens, FIXED_LL, FIXED_D, eob)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, eob=True, cl_lens=None, cl_syms=None, hclen=None, hlit=None, hdist=None):
        """BTYPE 10.  ll_lens / d_lens: the code lengths as the header lists them (257..286 and 1..30 entries; hlit / hdist
        override the COUNTS written, for headers that claim more than may be).  cl_syms: the run-length form of the two lists,
        [(symbol, extra value)], where the test wants the repeats just so; cl_lens: the 19 lengths of the code length code;
        hclen: how many of them are written (4..19)."""
        lens = list(ll_lens) + list(d_lens)
        syms = rle_code_lengths(lens) if cl_syms is None else list(cl_syms)
        if cl_lens is None:
            freq = [0] * 19
            for s, _ in syms:
                freq[s] += 1
            cl_lens = limited_lengths(freq, 7)
            if sum(1 for l in cl_lens if l) == 1:  # (a single code length code would be incomplete: give it a partner)
                cl_lens[[s for s in (0, 18) if not cl_lens[s]][0]] = 1
        assert len(cl_lens) == 19
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CLORDER[i]]])
        assert 4 <= hclen <= 19 and all(cl_lens[CLORDER[i]] == 0 for i in range(hclen, 19))
        self.w.bits(int(final), 1)
        self.w.bits(2, 2)
        self.w.bits((len(ll_lens) if hlit is None else hlit) - 257, 5)
        self.w.bits((len(d_lens) if hdist is None else hdist) - 1, 5)
        self.w.bits(hclen - 4, 4)
        for i in range(hclen):
            self.w.bits(cl_lens[CLORDER[i]], 3)
        cl_codes = canonical(cl_lens)
        for s, extra in syms:
            assert cl_lens[s], ("code length symbol without a code", s)
            self.w.code(cl_codes[s], cl_lens[s])
            if s >= 16:
                self.w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
        self.header_end = self.w.bitpos
        self._tokens(tokens, list(ll_lens), list(d_lens), eob)
        return self

    def auto_dynamic(self, tokens, final=False, min_hlit=257, min_hdist=1):
        """A dynamic block whose code lengths are derived from the tokens (length-limited Huffman, 15 bits)."""
        lf, df = [0] * 286, [0] * 30
        lf[256] = 1
        for t in tokens:
            if isinstance(t, int):
                lf[t] += 1
            else:
                lf[t.lsym if t.lsym is not None else length_symbol(t.length)[0]] += 1
                df[dist_symbol(t.dist)[0]] += 1
        ll, dl = limited_lengths(lf, 15), limited_lengths(df, 15)
        hlit = max(min_hlit, max(i for i in range(286) if ll[i]) + 1)
        hdist = max([min_hdist] + [i + 1 for i in range(30) if dl[i]])
        return self.dynamic(tokens, ll[:hlit], dl[:hdist], final=final)

    def _tokens(self, tokens, ll_lens, d_lens, eob):
        llc, dc = canonical(ll_lens), canonical(d_lens)
        w = self.w

        def ll(sym):
            assert sym < len(ll_lens) and ll_lens[sym], ("literal/length symbol without a code", sym)
            w.code(llc[sym], ll_lens[sym])

        def dd(sym):
            assert sym < len(d_lens) and d_lens[sym], ("distance symbol without a code", sym)
            w.code(dc[sym], d_lens[sym])

        for t in list(tokens) + ([EOB] if eob else []):
            if isinstance(t, int):
                ll(t)
                self.out.append(t)
            elif t == EOB:
                ll(256)
            elif isinstance(t, RawLL):
                ll(t.sym)
            else:
                length = t.length
                if isinstance(t, M) and t.lsym is not None:
                    sym, eb = t.lsym, LEXT[t.lsym - 257]
                    ev = length - LBASE[sym - 257]
                    assert 0 <= ev < (1 << eb) or (eb == 0 and ev == 0), ("length does not fit the symbol", length, sym)
                else:
                    sym, eb, ev = length_symbol(length)
                ll(sym)
                w.bits(ev, eb)
                if isinstance(t, RawDist):
                    dd(t.dsym)
                    continue
                ds, deb, dev = dist_symbol(t.dist)
                dd(ds)
                w.bits(dev, deb)
                self._copy(length, t.dist)

    # ---- padding: the next block starts at a chosen bit of its byte ----
    def pad_to_bit(self, bit):
        """Empty fixed blocks (10 bits each) until the position is `bit` (mod 8)."""
        while self.w.bitpos % 8 != bit % 8:
            self.fixed([])
        return self

    def finish(self, trailing=b""):
        return self.w.getvalue() + trailing


def cut_bits(stream, nbits):
    """The first nbits bits of a stream: whole bytes, the last one with its upper bits cleared."""
    out = bytearray(stream[:(nbits + 7) // 8])
    if nbits % 8:
        out[-1] &= (1 << (nbits % 8)) - 1
    return bytes(out)
