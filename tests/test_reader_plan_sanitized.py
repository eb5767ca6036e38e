"""The file reader's host planning under AddressSanitizer + UBSan on the CPU: tests/hostcheck/reader_plan_check.cpp compiles
orc_rust_amd/csrc/orcgpu_reader_plan.inc -- the text liborcgpu.so is built from -- into a stand-alone program.  The projection
walk, the stripe plan (selection, row-group ranges, pieces, entries, the column fill) and the grouping policy must equal field by
field what the blocks gave that the reader file held before (kept in the program), over seeded random inputs and the edge cases
written out by hand there.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g1", "-O0"]
CASES = [
    'projection, random',
    'projection, by name, by index, all',
    'projection, fewer schema fields than columns',
    'projection, a hint that mismatches at depth 0 and at depth 2',
    'projection, Map with and without the sorted flag',
    'projection, a List with two subtypes',
    'projection, a type cycle at kMaxTypeDepth',
    'projection, a column shard over 2 and 4 ranks',
    'projection, a dictionary column that is not projected, with and without column sharding',
    'projection, the stripe shard rule',
    'plan, random',
    'plan, stride 0',
    'plan, one row group',
    'plan, n_rows an exact multiple of the stride and one more',
    'plan, a selection that keeps nothing, everything, the first, the last, every other group; with and without a row filter',
    'plan, predicate keep-lists that merge neighbours',
    'plan, a predicate that fails and therefore selects all',
    'plan, predicate and selection intersected',
    "plan, another rank's stripe consuming its share of the selection",
    'plan, a batch that straddles a group boundary',
    'plan, batch_size equal to the stride and coprime with it',
    'pieces, uncompressed, with and without a non-zero skip_bytes',
    'pieces, compressed: the second header missing, a header length past the stream, an entry beyond the stream',
    'pieces, skip_values 512 and 513',
    'pieces, skip_bits 7 and 8',
    'pieces, an index with the wrong n_groups',
    "pieces, a dictionary column's LENGTH and DICTIONARY_DATA streams",
    'pieces, e1.chunk_offset < e0.chunk_offset',
    'entries, a stream just under and exactly at 16384 bytes per group',
    'entries, a bad entry that clears the list',
    'grouping, the stager has room: queue sizes and byte totals at each constant and one below; prefetch 1, 2, 4',
    'grouping, the decoder should wake: pieces only against mixed',
    'grouping, the next staged piece joins this group',
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reader_plan") / "reader_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "reader_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout.splitlines()


def test_planning_equals_the_blocks_it_was_taken_from(lines):
    assert lines[-1] == "checked %d cases, 0 mismatches" % len(CASES), lines[-3:]
    assert [ln.rsplit(": ", 2)[0] for ln in lines[:-1]] == CASES
    assert all(ln.endswith(": same") for ln in lines[:-1]), [ln for ln in lines if not ln.endswith(": same")]


def test_random_cases_are_thousands(lines):
    sizes = {ln.rsplit(": ", 2)[0]: ln.rsplit(": ", 2)[1] for ln in lines[:-1]}
    assert sizes["projection, random"] == "3000 calls" and sizes["plan, random"] == "4000 calls"
