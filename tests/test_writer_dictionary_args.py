"""ArrowWriterBuilder.with_dictionary_key_size_threshold: the argument is checked in Python, before anything reaches the GPU."""
import pyarrow as pa
import pytest

from orc_rust_amd import ArrowWriter, ArrowWriterBuilder, capi

SCHEMA = pa.schema([("s", pa.string())])


@pytest.mark.parametrize("t", ["0.5", None, True, False, float("nan"), -0.1, -1, 1.5, 2, float("inf"), [0.5]])
def test_bad_threshold_is_a_value_error(t):
    with pytest.raises(ValueError):
        ArrowWriterBuilder("unused.orc", SCHEMA).with_dictionary_key_size_threshold(t)


@pytest.mark.parametrize("t", [0, 0.0, 1, 1.0, 0.8, 1e-9])
def test_thresholds_chain(t):
    b = ArrowWriterBuilder("unused.orc", SCHEMA)
    assert b.with_dictionary_key_size_threshold(t) is b


def test_entry_points_exist():
    assert "orcgpu_writer_set_dictionary" in capi.EXPORTS and "orcgpu_writer_dictionary_counts" in capi.EXPORTS
    assert callable(ArrowWriter.dictionary_counts)
