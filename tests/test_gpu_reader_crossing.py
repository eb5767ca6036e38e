"""The file reader across its planning paths on one file: 3 stripes of 5 000 rows, row groups of 1 000, written by pyarrow with
Zstandard and uncompressed; an int64, a double with nulls, a string, a decimal and a struct of two ints.  Read serially and with
read-ahead under a row selection that cuts stripes into pieces (row groups 1 and 3 of stripe 0, nothing of stripe 1, one row of the
last row group of stripe 2), a predicate that keeps the middle stripe, the selection with a row filter, the selection with
COUNT / SUM, and stripe shards over two ranks.  Rows, rows_seen / rows_kept and row_groups(read, total) are worked out from the
pyarrow table in plain Python."""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

STRIPE, STRIDE, N = 5000, 1000, 15000
FLAT = ["id", "d", "s", "dec"]
# rows [1000, 2000) and [3000, 4000) of stripe 0, nothing of stripe 1, row 14 500 (the last row group of stripe 2)
SELECTION = [(1000, True), (1000, False), (1000, True), (1000, False), (1000 + STRIPE + 4500, True), (1, False), (499, True)]
SELECTED = list(range(1000, 2000)) + list(range(3000, 4000)) + [14500]
_CTX = None


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(5)
    return pa.table({
        "id": pa.array(np.arange(N), pa.int64()),
        "d": pa.array([None if i % 7 == 3 else i * 0.5 for i in range(N)], pa.float64()),
        "s": pa.array(["row %d %s" % (i, rng.bytes(24).hex()) for i in range(N)]),   # (incompressible: a stripe per 5 000 rows)
        "dec": pa.array([decimal.Decimal(i * 3 - 20000).scaleb(-2) for i in range(N)], pa.decimal128(15, 2)),
        "st": pa.array([{"a": i, "b": -i} for i in range(N)], pa.struct([("a", pa.int32()), ("b", pa.int32())])),
    })


@pytest.fixture(scope="module", params=["zstd", "uncompressed"])
def path(request, table, tmp_path_factory):
    capi.load()
    p = str(tmp_path_factory.mktemp("crossing") / ("three_%s.orc" % request.param))
    orc.write_table(table, p, compression=request.param, stripe_size=1024, row_index_stride=STRIDE, batch_size=STRIPE)
    f = orc.ORCFile(p)
    assert [f.read_stripe(i).num_rows for i in range(f.nstripes)] == [STRIPE] * 3
    return p


def read(builder):
    r = builder.build()
    batches = list(r)
    got = pa.Table.from_batches(batches) if batches else None
    out = got, r.row_groups(), r.filter_rows()
    r.close()
    return out


def same(got, want):
    """Column names and values; the reader's fields say `not null` where a column has no nulls, pyarrow's table does not"""
    return got.column_names == want.column_names and got.num_rows == want.num_rows and got.to_pydict() == want.to_pydict()


def builder(path, prefetch, names=None):
    b = ArrowReaderBuilder.try_new(path, ctx()).with_prefetch(prefetch).with_batch_size(1024)
    return b.with_projection(names) if names else b


@pytest.mark.parametrize("prefetch", [0, 2])
def test_selection_cuts_stripes_into_pieces(path, table, prefetch):
    got, groups, _ = read(builder(path, prefetch).with_row_selection(SELECTION))
    assert same(got, table.take(SELECTED))
    assert groups == (3, 15)   # (row groups 1 and 3 of stripe 0, the last of stripe 2; stripe 1 is gone through and not read)


@pytest.mark.parametrize("prefetch", [0, 2])
def test_predicate_keeps_the_middle_stripe(path, table, prefetch):
    pred = P.and_([P.gte("id", V.Int64(STRIPE)), P.lt("id", V.Int64(2 * STRIPE))])
    got, groups, _ = read(builder(path, prefetch).with_predicate(pred))
    assert same(got, table.slice(STRIPE, STRIPE))
    assert groups == (5, 15)


@pytest.mark.parametrize("prefetch", [0, 2])
def test_selection_with_a_row_filter(path, table, prefetch):
    pred = P.lt("id", V.Int64(3500))
    got, groups, rows = read(builder(path, prefetch, FLAT).with_row_selection(SELECTION).with_row_filter(pred, prune=False))
    keep = [i for i in SELECTED if i < 3500]
    assert same(got, table.select(FLAT).take(keep))
    assert rows == (len(SELECTED), len(keep))
    assert groups == (4, 15)   # (a row filter keeps a stripe one result: row groups 1 to 3 of stripe 0, and the last of stripe 2)


@pytest.mark.parametrize("prefetch", [0, 2])
def test_selection_with_count_and_sum(path, table, prefetch):
    specs = [Agg.count_rows(), Agg.count("d"), Agg.sum("id"), Agg.sum("dec")]
    r = builder(path, prefetch, FLAT).with_row_selection(SELECTION).aggregating_reader(specs)
    got = r.aggregate()
    rows, groups = r.filter_rows(), r.row_groups()
    r.close()
    sub = table.take(SELECTED)
    assert got == [len(SELECTED), len(SELECTED) - sub["d"].null_count, sum(SELECTED), sum(x.as_py() for x in sub["dec"])]
    assert rows == (len(SELECTED), len(SELECTED))
    assert groups == (3, 15)


@pytest.mark.parametrize("prefetch", [0, 2])
def test_stripe_shards_of_two_ranks_put_together(path, table, prefetch):
    parts, groups = [], []
    for rank in range(2):
        got, g, _ = read(builder(path, prefetch).with_shard(rank, 2).with_row_selection([(500, True), (N - 500, False)]))
        parts.append(got)
        groups.append(g)
    # rank 0: stripes 0 (rows 500 on: all five row groups hold selected rows) and 2; rank 1: stripe 1
    assert same(parts[0], pa.concat_tables([table.slice(500, STRIPE - 500), table.slice(2 * STRIPE, STRIPE)]))
    assert same(parts[1], table.slice(STRIPE, STRIPE))
    assert groups == [(10, 10), (5, 5)]
