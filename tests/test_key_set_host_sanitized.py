"""The host side of the key sets under AddressSanitizer + UBSan on the CPU: tests/hostcheck/key_set_check.cpp compiles
orc_rust_amd/csrc/orcgpu_key_set.inc, the set leaf of orcgpu_filter_plan.inc and the probe of device/filter_program.h -- the text
liborcgpu.so is built from -- into a stand-alone program that builds its own cases and prints one line per fact.  The slot count and
byte size per limit, a table laid out on the host in the sealed layout that answers in_probe_i64 with and without the hash-bits
mask, the compile of ORCGPU_PRED_IN_SET to FOP_IN_SET with its plane number, and the refusals with their statuses and messages.
No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, UNSUPPORTED, INVALID = 0, 7, 101
FOP_FALSE, FOP_AND, FOP_NOT, FOP_IN, FOP_IN_SET = 9, 10, 12, 14, 16
IN_HAS_NULL = 1
TABLE_7, TABLE_8, BYTES = 0x7f0000001000, 0x7f0000002000, 32 + 8 + 64 * 8


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("key_set_host") / "key_set_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "key_set_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[f[0]] = (f[1:], msg)
    return got


def ints(out, name):
    return [int(x) for x in out[name][0]]


def test_slots_and_bytes_per_limit(out):
    # ok, slots (the power of two >= 2 x max_keys, at least 64), where the occupancy and the slots begin, the table's bytes, the allocation's
    def lay(slots):
        table = 32 + slots // 64 * 8 + slots * 8
        return [1, slots, 32, 32 + slots // 64 * 8, table, (table + 255) // 256 * 256 + 256]
    assert ints(out, "lay_1") == lay(64)
    assert ints(out, "lay_32") == lay(64)
    assert ints(out, "lay_33") == lay(128)
    assert ints(out, "lay_max") == lay(1 << 27)
    assert ints(out, "lay_max")[4] < 2 ** 32            # what FilterInsn::lit_len and InTable::bytes carry
    assert ints(out, "lay_0")[0] == 0 and ints(out, "lay_over")[0] == 0
    # ORCGPU_KEY_SET_HASH_BITS: unset, empty, 1, 4, 32, 0
    assert ints(out, "mask") == [2 ** 32 - 1, 2 ** 32 - 1, 1, 15, 2 ** 32 - 1, 2 ** 32 - 1]


def test_a_table_in_the_sealed_layout_answers_the_probe(out):
    # built, slots, keys found, absent keys found, the longest run of occupied slots, then the header: kind, n_keys, flags, hash mask
    assert ints(out, "probe_300")[:4] == [1, 2048, 300, 0] and ints(out, "probe_300")[5:] == [0, 300, 0, 2 ** 32 - 1]
    assert ints(out, "probe_300")[4] < 20
    # under 1 and 4 hash bits every key starts in slot 0 / 1 or 0 .. 15: chains as long as the set, the same membership
    assert ints(out, "probe_300_bits1") == [1, 2048, 300, 0, 300, 0, 300, 0, 1]
    assert ints(out, "probe_300_bits4") == [1, 2048, 300, 0, 300, 0, 300, 0, 15]
    # INT64_MIN, INT64_MAX, 0, -1 and the value a free slot holds while the set is built
    assert ints(out, "probe_edge")[:4] == [1, 64, 5, 0] and ints(out, "probe_edge")[6] == 5
    assert ints(out, "probe_full_32")[:4] == [1, 64, 32, 0]
    assert ints(out, "probe_33_of_32")[0] == 0                                             # more keys than the limit: no table
    assert ints(out, "probe_none")[:4] == [1, 64, 0, 0]


def insns(out, name):
    f = out[name][0]
    assert int(f[0]) == OK, out[name]
    return [tuple(int(x) for x in k.split(":")) for k in f[1:] if ":" in k], [k for k in f[1:] if "=" in k]


def test_op_26_compiles_to_fop_in_set_with_its_plane(out):
    # op, cmp (IN_* flags), column, i (the plane), lo (FKIND_INT = 0), the table's address, its bytes
    assert insns(out, "set_i64") == ([(FOP_IN_SET, 0, 3, 0, 0, TABLE_7, BYTES)], ["leaves=1", "planes=1", "holds=1"])
    assert insns(out, "set_null_date") == ([(FOP_IN_SET, IN_HAS_NULL, 4, 0, 0, TABLE_8, BYTES)], ["leaves=1", "planes=1", "holds=1"])
    assert insns(out, "set_i8")[0] == [(FOP_IN_SET, 0, 0, 0, 0, TABLE_7, BYTES)]
    assert insns(out, "set_empty") == ([(FOP_FALSE, 0, 0, 0, 0, 0, 0)], ["leaves=0", "planes=0", "holds=0"])   # the empty set: FALSE, no plane
    prog, tail = insns(out, "mix")
    assert [p[0] for p in prog] == [FOP_IN, FOP_IN_SET, FOP_AND, FOP_IN_SET, FOP_NOT, FOP_AND]
    assert [p[3] for p in prog if p[0] in (FOP_IN, FOP_IN_SET)] == [0, 1, 2]                 # numbered with the IN planes, in leaf order
    assert prog[1][5:] == (TABLE_7, BYTES) and prog[3][1] == IN_HAS_NULL and prog[3][5:] == (TABLE_8, BYTES)
    assert tail == ["leaves=3", "planes=3", "holds=2"]
    # appended behind another plan: first instruction, op, plane (moved behind the IN list's), address and bytes (untouched), leaves, holds
    assert ints(out, "append") == [1, FOP_IN_SET, 1, TABLE_7, BYTES, 2, 1]
    assert ints(out, "hold_uses_after") == [1]                                            # every plan has let go of the sets' memory


def test_the_refusals_with_their_statuses_and_messages(out):
    for name, code, words in (("ref_ts", UNSUPPORTED, ("'ts'", "Timestamp")),
                              ("ref_tsi", UNSUPPORTED, ("'tsi'", "Timestamp")),
                              ("ref_dec", UNSUPPORTED, ("'dec'", "Decimal")),
                              ("ref_f64", UNSUPPORTED, ("'f64'", "Float")),
                              ("ref_bool", UNSUPPORTED, ("'b'", "Boolean")),
                              ("ref_string", UNSUPPORTED, ("'s'", "String")),
                              ("ref_unknown_column", INVALID, ("'nope'", "not a projected root column")),
                              ("ref_no_column", INVALID, ("without a column name",)),
                              ("ref_unsealed", INVALID, ("'i64'", "not sealed")),
                              ("ref_failed", INVALID, ("'i64'", "limit of 32", "unusable")),
                              ("ref_other_context", INVALID, ("'i64'", "12345", "not a set of this context")),
                              ("ref_no_sets", INVALID, ("not a set of this context",)),
                              ("ref_children", INVALID, ("'i64'", "children"))):
        assert ints(out, name) == [code], (name, out[name])
        assert out[name][1].startswith("row filter:"), out[name][1]
        for w in words:
            assert w in out[name][1], (name, out[name][1])
    assert ints(out, "col_dict") == [UNSUPPORTED] and "'d'" in out["col_dict"][1] and "dictionary column" in out["col_dict"][1]
    assert ints(out, "col_nested") == [UNSUPPORTED] and "'st'" in out["col_nested"][1] and "nested" in out["col_nested"][1]
    assert ints(out, "col_ok") == [OK]
