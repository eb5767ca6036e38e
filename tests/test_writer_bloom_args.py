"""ArrowWriterBuilder.with_bloom_filter_columns: the arguments are checked in Python, before anything reaches the GPU."""
import pyarrow as pa
import pytest

from orc_rust_amd import ArrowWriterBuilder, capi

SCHEMA = pa.schema([("k", pa.int64()), ("s", pa.string())])


@pytest.fixture(autouse=True)
def no_context(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a GPU context was opened")
    monkeypatch.setattr(capi, "Context", refuse)


@pytest.mark.parametrize("columns", ["k", ("k",), None, [b"k"], ["k", 1], {"k"}, 7])
def test_columns_not_a_list_of_str(columns):
    with pytest.raises(ValueError):
        ArrowWriterBuilder("unused.orc", SCHEMA).with_row_index_stride(10000).with_bloom_filter_columns(columns)


@pytest.mark.parametrize("fpp", ["0.01", None, True, [0.01], 0, 0.0, 1, 1.0, -0.5, 1.5, float("nan"), float("inf")])
def test_bad_fpp(fpp):
    with pytest.raises(ValueError):
        ArrowWriterBuilder("unused.orc", SCHEMA).with_row_index_stride(10000).with_bloom_filter_columns(["k"], fpp=fpp)


def test_stride_missing_at_try_build():
    b = ArrowWriterBuilder("unused.orc", SCHEMA).with_bloom_filter_columns(["k", "s"], fpp=0.01)
    with pytest.raises(ValueError):
        b.try_build()
    b = ArrowWriterBuilder("unused.orc", SCHEMA).with_bloom_filter_columns(["k"]).with_row_index_stride(0)
    with pytest.raises(ValueError):
        b.try_build()


@pytest.mark.parametrize("fpp", [0.01, 0.5, 1e-9, 0.999])
def test_chains(fpp):
    b = ArrowWriterBuilder("unused.orc", SCHEMA)
    assert b.with_bloom_filter_columns(["k"], fpp=fpp) is b
    assert b.with_bloom_filter_columns([]) is b


def test_entry_point_exists():
    assert "orcgpu_writer_set_bloom_filter" in capi.EXPORTS
