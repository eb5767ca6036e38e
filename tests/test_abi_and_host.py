"""CPU-side checks (no GPU): the C-ABI library builds for gfx950, loads, and exports every symbol
that include/orcgpu.h declares; without a HIP device the product fails loudly instead of falling
back to a CPU path; the multi-GPU sharding helpers and their only collective (an all-gather of row
counts) work across two gloo processes."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from orc_rust_amd import capi
    L = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orcgpu.h")).read()
    declared = sorted(set(re.findall(r"\b(orcgpu_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 15
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
    assert sorted(capi.EXPORTS) == declared
    assert b"gfx950" in L.orcgpu_version()


def test_code_object_targets_gfx950():
    from orc_rust_amd import capi
    so = capi.lib_path()
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", so], capture_output=True, text=True)
    blob = open(so, "rb").read()
    assert b"gfx950" in blob
    assert out.returncode == 0


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from orc_rust_amd import capi
    with pytest.raises(capi.OrcGpuError) as e:
        capi.Context(0)
    assert e.value.code == 100


def test_product_never_imports_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "orc_rust_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".inc", ".c", ".cpp")):
                text = open(os.path.join(base, f), errors="ignore").read()
                assert "oracle_lib" not in text and "liborc_oracle" not in text and "orc_oracle.h" not in text, f


def test_row_index_positions_are_dealt_out_by_stream():
    """orcgpu_index_entry (host only): one RowIndexEntry's positions (row_index.rs:42-50) split over the column's streams in the
    order PRESENT, DATA, LENGTH | SECONDARY, with the forms the ORC specification gives each stream kind."""
    import ctypes as C
    from orc_rust_amd import capi
    L = capi.load()

    def entry(orc_type, encoding, has_present, compressed, positions, kind):
        col = capi.Column()
        col.orc_type, col.encoding = orc_type, encoding
        pos = (C.c_uint64 * max(1, len(positions)))(*positions)
        out = capi.StreamEntry()
        rc = L.orcgpu_index_entry(C.byref(col), int(has_present), int(compressed), pos, len(positions), kind, C.byref(out))
        return rc, (out.chunk_offset, out.skip_bytes, out.skip_values, out.skip_bits)

    PRESENT, DATA, LENGTH, SECONDARY = 0, 1, 2, 5
    LONG, STRING, BOOLEAN, DOUBLE, DECIMAL, TIMESTAMP, STRUCT = 4, 7, 0, 6, 14, 9, 12
    # Long, compressed, with PRESENT: 4 + 3 positions
    p = [100, 7, 3, 0, 2000, 11, 5]
    assert entry(LONG, 2, True, True, p, PRESENT) == (0, (100, 7, 3, 0))
    assert entry(LONG, 2, True, True, p, DATA) == (0, (2000, 11, 5, 0))
    assert entry(LONG, 2, True, True, p[:6], DATA)[0] == 2       # OutOfSpec: one position short
    assert entry(LONG, 2, False, True, p, DATA)[0] == 2          # ... four too many for a column without PRESENT
    # uncompressed: {byte, run offset}
    assert entry(LONG, 2, False, False, [4096, 17], DATA) == (0, (4096, 0, 17, 0))
    # direct string: DATA = bytes only, LENGTH = run-length; dictionary string: DATA = run-length keys, nothing for LENGTH
    assert entry(STRING, 2, False, True, [10, 20, 30, 40, 50], DATA) == (0, (10, 20, 0, 0))
    assert entry(STRING, 2, False, True, [10, 20, 30, 40, 50], LENGTH) == (0, (30, 40, 50, 0))
    assert entry(STRING, 3, False, True, [10, 20, 30], DATA) == (0, (10, 20, 30, 0))
    assert entry(STRING, 3, False, True, [10, 20, 30], LENGTH)[0] == 101  # InvalidArgument: the dictionary's lengths have no positions
    # Boolean: bits over byte runs; Double: bytes; Decimal: bytes + scales; Timestamp: two run-length streams; Struct: PRESENT only
    assert entry(BOOLEAN, 0, False, False, [9, 2, 5], DATA) == (0, (9, 0, 2, 5))
    assert entry(DOUBLE, 0, True, False, [1, 0, 0, 800], DATA) == (0, (800, 0, 0, 0))
    assert entry(DECIMAL, 2, False, True, [1, 2, 3, 4, 5], SECONDARY) == (0, (3, 4, 5, 0))
    assert entry(TIMESTAMP, 2, False, False, [1, 2, 3, 4], SECONDARY) == (0, (3, 0, 4, 0))
    assert entry(STRUCT, 0, True, True, [1, 2, 3, 4], PRESENT) == (0, (1, 2, 3, 4))
    assert entry(STRUCT, 0, False, True, [], PRESENT)[0] == 101


def test_sharding_helpers():
    from orc_rust_amd import shard
    assert shard.stripe_shard(12, 1, 8) == [1, 9]
    assert sorted(sum([shard.stripe_shard(12, r, 8) for r in range(8)], [])) == list(range(12))
    costs = [8, 8, 8, 4, 16, 16, 16, 16, 1, 1, 4, 4, 4, 25, 10, 44]  # lineitem-like bytes/row
    parts = shard.column_shard(costs, 8)
    assert sorted(sum(parts, [])) == list(range(16))
    loads = [sum(costs[i] for i in p) for p in parts]
    assert max(loads) == 44 and min(loads) >= 16


def test_unit_shard_balances_and_covers():
    from orc_rust_amd import shard
    costs = [8, 8, 8, 4, 16, 16, 16, 16, 5, 5, 4, 4, 4, 16, 8.3, 30.5]
    stripe_rows = [2_189_312] * 21 + [2_034_168]
    for world in (1, 2, 4, 8):
        units, loads = shard.unit_shard(stripe_rows, costs, world)
        shard.check_unit_coverage(units, len(stripe_rows), len(costs))
        assert max(loads) <= 1.02 * (sum(loads) / world)
    offs, total = shard.stripe_row_offsets(stripe_rows)
    assert offs[1] == 2_189_312 and total == sum(stripe_rows)


_BENCH_WORKER = r"""
import os, sys, types
sys.path.insert(0, %r)
import torch.distributed as dist
import bench
from orc_rust_amd import shard
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
# the multi-rank path of bench.py up to the point where a GPU is needed: this rank's units, their stripes, the all-gather
args = types.SimpleNamespace(workload="lineitem", rows=30000, sf=0.0, scaling="weak", compression="none", full=True)
stripes, comp, label, desc, plan = bench.build_workload(args, rank, world)
assert plan["rows"] == 30000 * world and plan["n_columns"] == 16
unit_rows = sum(n * len(cols) for n, cols, _, _, _ in stripes)
allc = shard.gather_counts([unit_rows, 0, 0, sum(len(b) for _, _, st, _, _ in stripes for _, _, b in st), len(plan["units"]), 0], dist)
assert sum(c[4] for c in allc) == plan["n_stripes"] * 16
assert sum(c[0] for c in allc) == plan["rows"] * 16
allu = [None] * world
dist.all_gather_object(allu, plan["units"])
shard.check_unit_coverage(allu, plan["n_stripes"], 16)
# every rank holds only the columns of its units
for (n, cols, streams, expect, sums), s_ in zip(stripes, sorted({u[0] for u in plan["units"]})):
    assert sorted(c["column_id"] - 1 for c in cols) == sorted(c for s2, c in plan["units"] if s2 == s_)
    assert sorted(sums) == sorted(c["column_id"] for c in cols)
# strong scaling: the table does not grow with the ranks
args.scaling = "strong"
assert bench.build_workload(args, rank, world)[4]["rows"] == 30000
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_bench_starts_its_own_ranks_without_a_launcher():
    """`python bench.py --gpus 2` with no WORLD_SIZE: bench.py starts both ranks itself (fresh children, the parent never
    touches the GPU), they rendezvous over gloo and get as far as orcgpu_open -- which fails here (no GPU in this
    container) with the library's own message; on a GPU box the same path carries on to the decode."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["BENCH_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "30000", "--compression", "none", "--no-cpu",
                        "--steps", "1", "--warmup", "0"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    import torch
    if torch.cuda.is_available():
        assert p.returncode == 0, err
        line = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert line["n_gpus"] == 2 and len(line["per_rank"]) == 2 and all(r["ms_per_step"] > 0 for r in line["per_rank"])
    else:
        assert p.returncode != 0
        assert "orcgpu_open" in err and "no usable HIP device" in err, err


def test_two_rank_gloo_bench_sharding(tmp_path):
    script = tmp_path / "bench_worker.py"
    script.write_text(_BENCH_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs


_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import torch.distributed as dist
from orc_rust_amd import shard
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
mine = shard.stripe_shard(12, rank, world)
rows = sum(8388608 if s < 11 else 7725312 for s in mine)
allc = shard.gather_counts([rows, len(mine), 0], dist)
offs, total = shard.global_row_offsets(allc)
assert total == 100_000_000, total
assert offs[0] == 0 and offs[1] == allc[0][0]
assert sum(c[1] for c in allc) == 12 and all(c[2] == 0 for c in allc)
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_two_rank_gloo_row_count_allgather(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs


# ---- the reader's shard spec (orcgpu_reader_set_shard; host logic: orcgpu_shard_columns) --------------------------------------
def _deal(weights, world):
    import ctypes as C
    from orc_rust_amd import capi
    L = capi.load()
    w = (C.c_double * len(weights))(*weights)
    out = (C.c_uint32 * max(1, len(weights)))()
    assert L.orcgpu_shard_columns(w, len(weights), world, out) == 0
    return [out[i] for i in range(len(weights))]


def test_column_deal_is_the_longest_processing_time_rule():
    lineitem = [8, 8, 8, 4, 16, 16, 16, 16, 20, 20, 4, 4, 4, 20, 20, 20]  # orcgpu_reader_column_weight of the 16 lineitem columns
    for world in (1, 2, 3, 4, 8, 16, 32):
        r = _deal(lineitem, world)
        assert all(0 <= x < world for x in r)
        load = [sum(w for w, x in zip(lineitem, r) if x == k) for k in range(world)]
        # the rule's own guarantee: no rank above the mean by more than the heaviest column
        assert max(load) <= sum(lineitem) / world + max(lineitem)
        # a restatement in Python: falling weight (ties: earlier first), to the least loaded rank (ties: the lower)
        ref_load, ref = [0.0] * world, [0] * len(lineitem)
        for i in sorted(range(len(lineitem)), key=lambda i: (-lineitem[i], i)):
            k = min(range(world), key=lambda k: (ref_load[k], k))
            ref[i] = k
            ref_load[k] += lineitem[i]
        assert r == ref
    assert _deal([], 4) == []


_SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import torch.distributed as dist
from test_abi_and_host import _deal
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
weights = [8, 8, 8, 4, 16, 16, 16, 16, 20, 20, 4, 4, 4, 20, 20, 20]
mine = [i for i, r in enumerate(_deal(weights, world)) if r == rank]              # ORCGPU_SHARD_COLUMNS
stripes = [k for k in range(35) if k %% world == rank]                            # ORCGPU_SHARD_STRIPES
everyone = [None] * world
dist.all_gather_object(everyone, (mine, stripes))
cols = sorted(c for m, _ in everyone for c in m)
assert cols == list(range(16)), cols                                             # every column exactly once
assert sorted(s for _, st in everyone for s in st) == list(range(35))            # every stripe exactly once
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_two_rank_gloo_reader_shards_partition_the_file(tmp_path):
    script = tmp_path / "shard_worker.py"
    script.write_text(_SHARD_WORKER % (ROOT, ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
