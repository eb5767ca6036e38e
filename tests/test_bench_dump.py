"""bench.py --dump-outputs on the host: which batches the sample takes, the 64 MB bound, and every Arrow layout of the bench
workloads as float arrays.  The CPU oracle's batches stand in for the device results: they have Result.batch's layout."""
import os

import numpy as np

import bench
import oracle_lib as O
from orc_rust_amd.gen import workloads as W


class _OracleResult:
    """What dump_outputs reads of a capi.Result (n_batches, batch(b, ci), view(b, ci).length), decoded by the oracle."""

    class _View:
        def __init__(self, length):
            self.length = length

    def __init__(self, n, cols, streams, compression, batch=8192):
        self.parts = []
        for c in cols:
            sd = {k: (b.tobytes() if isinstance(b, np.ndarray) else bytes(b)) for cid, k, b in streams if cid == c["column_id"]}
            oc = O.Column(c["orc_type"], c["encoding"], sd, dictionary_size=c.get("dictionary_size", 0), precision=c.get("precision", 0),
                          scale=c.get("scale", 0), compression=compression)
            assert oc.status == O.OK
            got = [oc.next_batch(min(batch, n - lo)) for lo in range(0, n, batch)]
            assert all(p["status"] == O.OK for p in got)
            oc.close()
            self.parts.append(got)
        self.n_batches = len(self.parts[0])

    def batch(self, b, ci):
        return self.parts[ci][b]

    def view(self, b, ci):
        return self._View(self.parts[ci][b]["length"])


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_lineitem_dump_holds_the_sampled_batches_as_the_generator_made_them(tmp_path):
    rows, cut = 50_000, 30_000
    table = W.lineitem_table(rows)
    stripes, results = [], []
    for lo, hi in ((0, cut), (cut, rows)):
        n, cols, streams, _ = W.lineitem_stripe(table, lo, hi, "zstd", want_expect=False)
        stripes.append((n, cols, streams, {}, None))
        results.append(_OracleResult(n, cols, streams, "zstd"))
    bench.dump_outputs(str(tmp_path / "a"), stripes, results)
    got = _load(str(tmp_path / "a"))
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= bench.DUMP_BYTES
    taken = got.pop("batches").astype(np.int64)
    # every batch fits the budget here: the first and the last come first, then all the others in the seeded order
    assert len(taken) == 4 + 3 and tuple(taken[0]) == (0, 0, 8192) and tuple(taken[1]) == (1, 2, 20_000 - 2 * 8192)
    assert sorted(map(tuple, taken[:, :2])) == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2)]
    first_rows = [(0, cut)[k] + b * 8192 for k, b, _ in taken]
    sel = np.concatenate([np.arange(r0, r0 + m) for r0, (_, _, m) in zip(first_rows, taken)])
    for name, typ, how in W.LINEITEM:
        if how in ("i64", "i32", "dec"):
            assert got[name].dtype == np.float64
            assert np.array_equal(got[name], table[name][sel].astype(np.float64)), name
        else:
            if how == "dict":
                words = W.DICTS[name]
                lens = np.array([len(words[k]) for k in table[name][sel]])
                text = b"".join(words[k] for k in table[name][sel])
            else:
                clen, cbytes = table[name]
                starts = np.concatenate(([0], np.cumsum(clen, dtype=np.int64)))
                lens = clen[sel]
                text = b"".join(cbytes[starts[i]:starts[i + 1]].tobytes() for i in sel)
            offs = got[name + ".offsets"]
            assert offs.dtype == np.float64 and offs.size == sel.size + len(taken)
            assert np.array_equal(np.concatenate([np.diff(o) for o in np.split(offs, np.cumsum(taken[:, 2] + 1)[:-1])]), lens), name
            assert got[name + ".bytes"].dtype == np.float32
            assert got[name + ".bytes"].astype(np.uint8).tobytes() == text, name
    assert not any(k.endswith(".validity") for k in got)
    # the same results give the same files; a smaller budget keeps a prefix of the same order
    bench.dump_outputs(str(tmp_path / "b"), stripes, results)
    again = _load(str(tmp_path / "b"))
    assert again.keys() == got.keys() | {"batches"} and all(np.array_equal(again[k], got[k]) for k in got)
    bench.dump_outputs(str(tmp_path / "c"), stripes, results, budget=8 << 20)
    small = _load(str(tmp_path / "c"))
    assert 1 <= len(small["batches"]) < len(taken) and np.array_equal(small["batches"], taken[:len(small["batches"])])
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "c"), f)) for f in os.listdir(str(tmp_path / "c"))) <= 8 << 20


def test_nulls_timestamps_and_ranks(tmp_path):
    n, cols, streams, expect = W.c3_stripe(20_000, 0, "none")
    res = _OracleResult(n, cols, streams, "none")
    bench.dump_outputs(str(tmp_path / "c3"), [(n, cols, streams, {}, None)], [res], rank=1, world=2)
    got = _load(str(tmp_path / "c3"))
    assert set(got) == {"rank1.batches", "rank1.shipmode.offsets", "rank1.shipmode.bytes", "rank1.shipmode.validity"}
    taken = got["rank1.batches"].astype(np.int64)
    sel = np.concatenate([np.arange(b * 8192, b * 8192 + m) for _, b, m in taken])
    assert np.array_equal(got["rank1.shipmode.validity"], expect[1]["present"][sel].astype(np.float32))
    lens = np.concatenate([np.diff(o) for o in np.split(got["rank1.shipmode.offsets"], np.cumsum(taken[:, 2] + 1)[:-1])])
    assert np.array_equal(lens, expect[1]["lengths"][sel])
    n, cols, streams, expect, _ = W.c5_stripe(9_000, 0, "lz4")
    bench.dump_outputs(str(tmp_path / "c5"), [(n, cols, streams, {}, None)], [_OracleResult(n, cols, streams, "lz4")])
    got = _load(str(tmp_path / "c5"))
    assert np.array_equal(got["ts"], np.frombuffer(expect[1]["values"], dtype=np.int64).astype(np.float64))


def test_column_arrays_of_every_fixed_width_layout():
    dec = np.array([[5, 0], [-7, -1], [0, 1], [-1, -2]], dtype=np.int64)  # 5, -7, 2^64, -2^64 - 1 as two's complement halves
    p = {"length": 4, "validity": None, "offsets": None, "values": dec.tobytes()}
    assert bench._column_arrays({"orc_type": W.DECIMAL}, p)["values"].tolist() == [5.0, -7.0, 2.0 ** 64, -(2.0 ** 64) - 1]
    p = {"length": 3, "validity": bytes([0b101]), "offsets": None, "values": np.array([1.5, 99.0, -2.25]).tobytes()}
    out = bench._column_arrays({"orc_type": W.DOUBLE}, p)
    assert out["values"].tolist() == [1.5, 0.0, -2.25] and out["validity"].tolist() == [1, 0, 1]
    p = {"length": 10, "validity": None, "offsets": None, "values": bytes([0b1000_0011, 0b10])}
    assert bench._column_arrays({"orc_type": W.BOOLEAN}, p)["values"].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 0, 1]
    for dt, typ in ((np.int8, W.BYTE), (np.int16, W.SHORT), (np.int32, W.DATE), (np.float32, W.FLOAT)):
        v = np.array([-3, 0, 7], dtype=dt)
        p = {"length": 3, "validity": None, "offsets": None, "values": v.tobytes()}
        assert bench._column_arrays({"orc_type": typ}, p)["values"].tolist() == [-3.0, 0.0, 7.0]
