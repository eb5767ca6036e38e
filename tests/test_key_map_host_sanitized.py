"""The key maps' and lookup columns' host side under AddressSanitizer + UBSan on the CPU: tests/hostcheck/key_map_check.cpp compiles
orc_rust_amd/csrc/orcgpu_lookup_plan.inc and device/key_map_program.h -- the text liborcgpu.so is built from -- into a stand-alone
program.  The value planes' offsets and bytes, which columns may be a value, the lookup plan against a root table (order, pairs,
name clashes, every refusal with its status and a fragment of its message), and tables laid out on the host and probed with the
probe text the kernel runs, against tests/key_map_model.py -- with all of a key's hash and with a masked hash.  No GPU, nothing
loaded into Python."""
import os
import subprocess

import pytest

import key_map_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, UNSUPPORTED, INVALID = 0, 7, 101
INT64, DEC128, F64 = 0, 1, 2


def probe_case(n, seed):
    """n build rows: keys spread over int64 with the edges and the sentinel's value among them, an int and a float value, either
    of them NULL now and then; the probe keys: every build key, its neighbour, and the edges"""
    import random
    rng = random.Random(seed)
    keys = [M.SENTINEL, M.INT64_MIN, M.INT64_MAX, 0, -1][:n]
    while len(keys) < n:
        k = rng.choice((rng.randrange(-50, 50), rng.randrange(M.INT64_MIN, M.INT64_MAX)))
        if k not in keys:
            keys.append(k)
    rows = []
    for i, k in enumerate(keys):
        a = None if i % 5 == 1 else (k * 3) % (2 ** 63)
        b = None if i % 7 == 2 else (float(i) - 0.5 if i % 3 else -0.0)
        rows.append((a, b))
    probes = keys + [k + 1 for k in keys if k < M.INT64_MAX] + [M.SENTINEL, M.SENTINEL - 1, M.INT64_MIN, M.INT64_MAX]
    return keys, rows, probes


PROBES = {  # name: (max_keys, hash bits (0: all), case)
    "hand": (32, 0, ([1, 2, M.SENTINEL], [(10, None), (None, 1.0), (77, 7.5)], [1, 2, 3, M.SENTINEL, M.SENTINEL + 1])),
    "null_under_sentinel": (32, 0, ([M.SENTINEL], [(None, None)], [M.SENTINEL, 0])),
    "empty": (32, 0, ([], [], [0, M.SENTINEL])),
    "full_300": (300, 0, probe_case(300, 1)),
    "bits1_300": (300, 1, probe_case(300, 1)),
    "bits4_300": (300, 4, probe_case(300, 2)),
    "exactly_32_of_32": (32, 0, probe_case(32, 3)),
}


def probe_args(name):
    max_keys, bits, (keys, rows, probes) = PROBES[name]
    args = ["probe", name, str(max_keys), str(bits), str(len(keys))]
    for k, (a, b) in zip(keys, rows):
        args += [str(k), "n" if a is None else str(a), "n" if b is None else "%x" % M.bits(b)]
    return args + [str(p) for p in probes]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("key_map_host") / "key_map_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "key_map_check.cpp")])
    args = []
    for name in PROBES:
        args += probe_args(name)
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        if f[0] == "probe":
            got[("probe", f[1])] = (f[2:], msg)
        else:
            got[f[0]] = (f[1:], msg)
    return got


def test_plane_offsets_and_bytes(out):
    def planes(name):
        f, _ = out[name]
        return int(f[0]), int(f[1]), int(f[2]), int(f[3]), [tuple(int(x) for x in p.split(":")) for p in f[4:]]

    def up(x):
        return (x + 255) // 256 * 256

    # 1 key -> 64 slots; a plane holds slots + 1 entries (the sentinel's value has its own), every part 256-byte aligned
    assert planes("planes_1_i64") == (1, 64, up(65 * 8) + up(65), up(32 + 8 + 64 * 8) + 256 + up(65 * 8) + up(65), [(0, up(65 * 8))])
    ok, slots, bytes_, total, offs = planes("planes_32_mixed")
    a = up(65 * 8)
    b = a + up(65)
    c = b + up(65 * 16)
    d = c + up(65)
    assert (ok, slots, offs) == (1, 64, [(0, a), (b, c), (d, d + up(65 * 8))]) and bytes_ == d + up(65 * 8) + up(65)
    assert planes("planes_33_dec")[:3] == (1, 128, up(129 * 16) + up(129))
    ok, slots, bytes_, total, offs = planes("planes_1M_eight")
    per = up(((1 << 21) + 1) * 16) + up((1 << 21) + 1)
    assert (ok, slots, bytes_) == (1, 1 << 21, 8 * per) and [o[0] for o in offs] == [k * per for k in range(8)]
    assert total == bytes_ + up(32 + (1 << 21) // 8 + (1 << 21) * 8) + 256  # the set's table and control words, then the planes
    for name in ("planes_none", "planes_nine", "planes_0_keys"):
        assert planes(name)[0] == 0 and planes(name)[3] == 0, name


def test_which_columns_may_be_a_value(out):
    for name, kind in (("val_byte", INT64), ("val_date", INT64), ("val_float", F64)):
        assert out[name][0] == [str(OK), str(kind), "0", "0"], name
    assert out["val_dec"][0] == [str(OK), str(DEC128), "12", "2"]  # the column's own precision and scale
    for name, words in (("val_bool", "Boolean"), ("val_string", "String"), ("val_ts", "Timestamp"), ("val_dict", "String"), ("val_dict_int", "dictionary"),
                        ("val_nested", "nested")):
        f, msg = out[name]
        assert int(f[0]) == UNSUPPORTED and words in msg and "value column 'c'" in msg, (name, msg)
    assert int(out["names_twice"][0][0]) == INVALID and "'a' is given twice" in out["names_twice"][1]
    assert int(out["names_nine"][0][0]) == INVALID and "at most ORCGPU_KEY_MAP_MAX_VALUES (8)" in out["names_nine"][1]
    assert int(out["names_none"][0][0]) == INVALID and "no value column" in out["names_none"][1]
    assert int(out["names_eight"][0][0]) == OK


def plan(out, name):
    """status, [(name, pair, value, kind, precision, scale)], [(key column, map id, n columns)], message"""
    f, msg = out[name]
    rc, n, n_pairs = int(f[0]), int(f[1]), int(f[2])
    cols = [tuple(x if i == 0 else int(x) for i, x in enumerate(c.split(":"))) for c in f[3:3 + n]]
    pairs = [tuple(int(x) for x in p.split(":")) for p in f[3 + n:3 + n + n_pairs]]
    return rc, cols, pairs, msg


def test_the_plan_groups_columns_by_map_and_key(out):
    assert plan(out, "plan_one")[:3] == (OK, [("x", 0, 0, INT64, 0, 0)], [(3, 7, 1)])
    # three values of one map on one key: ONE pair, one probe per row
    assert plan(out, "plan_pair_shares_probe")[:3] == (OK, [("x", 0, 0, INT64, 0, 0), ("y", 0, 1, DEC128, 12, 2), ("z", 0, 2, F64, 0, 0)], [(3, 7, 3)])
    # the columns keep the order given, whichever pair serves them
    rc, cols, pairs, _ = plan(out, "plan_two_maps")
    assert rc == OK and [c[:2] for c in cols] == [("x", 0), ("y", 1), ("z", 0)] and pairs == [(3, 7, 2), (2, 8, 1)]
    assert plan(out, "plan_same_map_two_keys")[2] == [(0, 7, 1), (4, 7, 1)]  # Byte and Date keys; the same map twice is two pairs
    assert plan(out, "plan_with_computed")[:3] == (OK, [("x", 0, 0, INT64, 0, 0)], [(1, 7, 1)])
    rc, cols, pairs, _ = plan(out, "plan_eight")
    assert rc == OK and len(cols) == 8 and pairs == [(0, 7, 2), (1, 7, 2), (2, 8, 2), (3, 8, 2)]


def test_a_plan_shares_the_maps_memory(out):
    assert int(out["hold_uses"][0][0]) > 1 and int(out["hold_uses_after"][0][0]) == 1


REFUSALS = [
    ("ref_none", INVALID, "no lookup column given"), ("ref_nine", INVALID, "more than ORCGPU_LOOKUP_MAX (8)"), ("ref_empty_name", INVALID, "without a name"),
    ("ref_twice", INVALID, "the name 'x' is given twice"), ("ref_root_name", INVALID, "'i32' is the name of a root column of the file"),
    ("ref_root_name_unprojected", INVALID, "'unprojected' is the name of a root column of the file"), ("ref_computed_name", INVALID, "'c1' is the name of a computed column"),
    ("ref_no_map", INVALID, "names no key map"), ("ref_unsealed", INVALID, "not sealed yet"), ("ref_failed", INVALID, "more than max_keys keys"),
    ("ref_duplicate", INVALID, "duplicate key"), ("ref_other_context", INVALID, "another context"), ("ref_value_index", INVALID, "value 3 of a key map of 3 values"),
    ("ref_no_key", INVALID, "names no probe key column"), ("ref_unknown_key", INVALID, "'nope' is not a projected root column"),
    ("ref_unprojected_key", INVALID, "'unprojected' is not a projected root column"), ("ref_lookup_key", UNSUPPORTED, "its probe key 'x' is a lookup column"),
    ("ref_computed_key", UNSUPPORTED, "its probe key 'c1' is a computed column"), ("ref_ts_key", UNSUPPORTED, "column 'ts' is a Timestamp column"),
    ("ref_dec_key", UNSUPPORTED, "column 'dec' is a Decimal column"), ("ref_f64_key", UNSUPPORTED, "column 'f64' is a Float / Double column"),
    ("ref_bool_key", UNSUPPORTED, "column 'b' is a Boolean column"), ("ref_string_key", UNSUPPORTED, "column 's' is a String"),
    ("ref_dict_key", UNSUPPORTED, "column 'dict' is read as a dictionary column"), ("ref_nested_projection", UNSUPPORTED, "the projected column 's' is nested"),
    ("ref_fifth_pair", INVALID, "a fifth (key map, probe key) pair"),
]


@pytest.mark.parametrize("name,code,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_with_a_fragment_of_its_message(out, name, code, words):
    rc, cols, pairs, msg = plan(out, name)
    assert rc == code and words in msg and not cols and not pairs, (name, rc, msg)


def test_a_computed_column_over_a_lookup_column_says_so(out):
    f, msg = out["computed_over_lookup"]
    assert int(f[0]) == UNSUPPORTED and "computed column 'r': its operand 'x' is a lookup column" in msg and "not supported" in msg
    assert int(out["computed_over_file"][0][0]) == OK


@pytest.mark.parametrize("name", list(PROBES))
def test_a_table_laid_out_on_the_host_answers_the_model(out, name):
    _, _, (keys, rows, probes) = PROBES[name]
    m, _ = M.build(keys, rows)
    f, _ = out[("probe", name)]
    assert f[0] == "1" and len(f) == 1 + len(probes), (name, f[:3])
    want_a, want_b = M.probe(m, probes, 0), M.probe(m, probes, 1)
    for got, a, b, p in zip(f[1:], want_a, want_b, probes):
        assert got == "%s:%s" % ("n" if a is None else a, "n" if b is None else "%x" % M.bits(b)), (name, p, got)


def test_the_probe_cases_hold_the_edges():
    keys, rows, probes = PROBES["hand"][2]
    m, _ = M.build(keys, rows)
    assert [M.why_null(m, p, 0) for p in probes] == [None, "value", "absent", None, "absent"]
    keys, rows, probes = probe_case(300, 1)
    m, _ = M.build(keys, rows)
    assert M.SENTINEL in m and {M.why_null(m, p, 0) for p in probes} == {None, "value", "absent"} and M.bits(-0.0) in {M.bits(r[1]) for r in rows if r[1] is not None}
