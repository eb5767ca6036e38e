"""tests/writer_bloom_model.py against an outside yardstick: the BLOOM_FILTER_UTF8 streams Apache ORC wrote into
tests/golden/data/bloom_filter.orc (204 rows, zlib, stride 10000, fpp 0.01) for its Int, String, Double and Binary columns."""
import pytest

import arrow_util as A
import writer_bloom_model as BM
from orcfile import BLOOM_FILTER_UTF8, ROW_INDEX, OrcFile

FIXTURE_COLUMNS = ["id", "name", "score", "data"]  # (flag: a Boolean's filter there is not hash_long(0 / 1)'s; Date and Decimal: no model)


def test_sizing():
    assert BM.size(10000, 0.01) == (1498, 7)
    assert BM.size(1, 0.999) == (1, 1)  # (no bits asked for: one word, one function)
    words, k = BM.size(50000, 0.001)
    assert words * 8 > 48 << 10 and k == 10


@pytest.fixture(scope="module")
def fixture():
    return OrcFile(A.data_path("bloom_filter.orc")), A.expected_table("bloom_filter")


@pytest.mark.parametrize("name", FIXTURE_COLUMNS)
def test_model_reproduces_the_fixture(fixture, name):
    of, table = fixture
    assert of.row_index_stride == 10000 and [s.number_of_rows for s in of.stripes] == [204]
    cid = {n: c for n, c, _ in of.root_columns()}[name]
    (got,) = BM.file_streams(of, cid)
    (want,) = BM.column_streams(table.column(name), [204], 10000, 0.01)
    assert got == want
    (filt,) = BM.filters(got)
    assert filt[0] == 7 and len(filt[1]) == 1498
    for h in BM.hashes(table.column(name).combine_chunks()):
        assert BM.might_contain(filt, h)


def test_fixture_stream_order(fixture):
    of, _ = fixture
    index = [(k, c) for k, c, _ in of.stripes[0].stream_list if k in (ROW_INDEX, BLOOM_FILTER_UTF8)]
    assert index[0] == (ROW_INDEX, 0)
    assert index[1:] == [(k, c) for c in range(1, 8) for k in (ROW_INDEX, BLOOM_FILTER_UTF8)]
