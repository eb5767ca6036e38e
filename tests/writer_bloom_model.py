"""TEST INFRASTRUCTURE: the ArrowWriter's Bloom filters (orcgpu_writer_set_bloom_filter, ArrowWriterBuilder.with_bloom_filter_columns)
in plain Python -- Apache ORC's sizing, the hash of a value per Arrow type, and the bytes of a column's BLOOM_FILTER_UTF8 stream per
stripe -- over the hashing of tests/predicate_model.py (hash_long, murmur3_64, bloom_with), which restates src/bloom_filter.rs."""
import math
import struct

import pyarrow as pa

import oracle_lib as O
import predicate_model as PM
from orcfile import BLOOM_FILTER_UTF8

NAN_BITS = 0x7FF8000000000000  # Double.doubleToLongBits of every NaN


def size(stride, fpp):
    """(64-bit words, hash functions) of every filter: BloomFilter.java's optimalNumOfBits / optimalNumOfHashFunctions"""
    num_bits = int(-stride * math.log(fpp) / (math.log(2) * math.log(2)))
    return num_bits // 64 + 1, max(1, int(math.floor(num_bits / stride * math.log(2) + 0.5)))


def hashes(array):
    """the 64-bit hashes of an Arrow array's valid values, in row order (nulls are not hashed)"""
    t = array.type
    out = []
    for v in array:
        if not v.is_valid:
            continue
        if pa.types.is_integer(t):
            out.append(PM.hash_long(v.as_py()))
        elif pa.types.is_floating(t):
            x = v.as_py()  # (a float32 widens exactly)
            out.append(PM.hash_long(NAN_BITS if x != x else struct.unpack("<q", struct.pack("<d", x))[0]))
        elif pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t):
            out.append(PM.murmur3_64(v.as_buffer().to_pybytes() if v.as_buffer() is not None else b""))
        else:
            raise TypeError("no Bloom filter hash for %s" % t)
    return out


def stream(array, stride, words, k):
    """the BLOOM_FILTER_UTF8 stream of one stripe's rows of a column: a filter per row group, the short last one too"""
    groups = [array.slice(at, stride) for at in range(0, len(array), stride)]
    return PM.bloom_index([PM.bloom_with(hashes(g), k, words) for g in groups], utf8=True)


def column_streams(column, stripe_rows, stride, fpp):
    """[stripe] the stream's bytes for a table column cut into stripes of stripe_rows"""
    words, k = size(stride, fpp)
    col = column.combine_chunks() if isinstance(column, pa.ChunkedArray) else column
    out, at = [], 0
    for n in stripe_rows:
        out.append(stream(col.slice(at, n), stride, words, k))
        at += n
    return out


def plain(of, raw):
    """an index stream of an OrcFile as the writer framed it -> its protobuf bytes"""
    if not of.compression:
        return bytes(raw)
    st, out = O.stream_decompress(bytes(raw), of.compression_name, of.block_size)
    assert st == 0, st
    return bytes(out)


def file_streams(of, column_id):
    """[stripe] the decoded BLOOM_FILTER_UTF8 stream of a column, None where the stripe has none"""
    return [plain(of, s.streams[(column_id, BLOOM_FILTER_UTF8)]) if (column_id, BLOOM_FILTER_UTF8) in s.streams else None for s in of.stripes]


def filters(stream_bytes):
    """a decoded stream -> [(k, [u64 words])] per row group"""
    from orcfile import pb_fields
    out = []
    for f, wt, v in pb_fields(stream_bytes):
        assert (f, wt) == (1, 2)
        k, words = None, None
        for g, w2, x in pb_fields(v):
            if g == 1:
                k = x
            elif g == 3:
                words = list(struct.unpack("<%dQ" % (len(x) // 8), bytes(x)))
            else:
                raise AssertionError("BloomFilter field %d" % g)
        out.append((k, words))
    return out


def might_contain(filt, hash64):
    """BloomFilter::test_hash"""
    k, words = filt
    return all(words[b // 64] >> (b % 64) & 1 for b in PM.bloom_bits(hash64, k, len(words)))
