"""ArrowWriterBuilder.with_compression: the arguments are checked in Python, before anything reaches the GPU."""
import pyarrow as pa
import pytest

from orc_rust_amd import ArrowWriterBuilder, arrow_writer, capi

SCHEMA = pa.schema([("x", pa.int64())])


@pytest.mark.parametrize("codec", ["gzip", "zstd", "zlib", "lzo", "SNAPPY", "", 2])
def test_unknown_codec_is_a_value_error(codec):
    with pytest.raises(ValueError):
        ArrowWriterBuilder("unused.orc", SCHEMA).with_compression(codec)


@pytest.mark.parametrize("block_size", [0, -1, 1 << 23])
def test_block_size_out_of_range(block_size):
    with pytest.raises(ValueError):
        ArrowWriterBuilder("unused.orc", SCHEMA).with_compression("snappy", block_size)


def test_known_codecs_chain():
    for codec in (None, "none", "snappy", "lz4"):
        b = ArrowWriterBuilder("unused.orc", SCHEMA)
        assert b.with_compression(codec, (1 << 23) - 1) is b
    # the codes the C ABI takes (ORCGPU_COMP_*)
    assert {k: v for k, v in arrow_writer.COMPRESSIONS.items() if k} == {k: capi.COMP[k] for k in ("none", "snappy", "lz4")}
    assert arrow_writer.DEFAULT_COMPRESSION_BLOCK_SIZE == 262144


def test_entry_points_are_exported():
    assert "orcgpu_writer_set_compression" in capi.EXPORTS and "orcgpu_compress_stream" in capi.EXPORTS
