"""GROUP BY's key compiler, stripe merge and finish step under AddressSanitizer + UBSan on the CPU:
tests/hostcheck/group_plan_check.cpp compiles orc_rust_amd/csrc/orcgpu_group_plan.inc -- the text liborcgpu.so is built from -- into
a stand-alone program.  Every key kind of the table in include/orcgpu.h with its status and message; 0 / 1 / 4 / 5 keys and a
duplicate; the merge of stripes (the same key twice, new keys keeping first-appearance order, NULL / 0 / '' apart, a 64-byte
string key, the cap at 65536 and 65537); the key record -> orcgpu_group_key step.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
KEY_I64, KEY_DEC128, KEY_BOOL, KEY_STRING = range(4)
FKIND_INT, FKIND_FLOAT, FKIND_BOOL, FKIND_STRING, FKIND_OTHER, FKIND_DEC128 = range(6)
# column -> (key kind, FKIND_*, scale_or_unit), or the refusal
KEYS = {
    "i8": (KEY_I64, FKIND_INT, -1), "i16": (KEY_I64, FKIND_INT, -1), "i32": (KEY_I64, FKIND_INT, -1), "i64": (KEY_I64, FKIND_INT, -1),
    "i64_as_i16": (KEY_I64, FKIND_INT, -1), "date": (KEY_I64, FKIND_INT, -1), "b": (KEY_BOOL, FKIND_BOOL, -1),
    "ts": (KEY_I64, FKIND_INT, 3), "ts_us": (KEY_I64, FKIND_INT, 2), "tsi": (KEY_I64, FKIND_INT, 3),
    "dec15_2": (KEY_DEC128, FKIND_DEC128, 2), "dec38_0": (KEY_DEC128, FKIND_DEC128, 0),
    "s": (KEY_STRING, FKIND_STRING, -1), "vc": (KEY_STRING, FKIND_STRING, -1), "ch": (KEY_STRING, FKIND_STRING, -1),
    "f32": -MISMATCHED, "f64": -MISMATCHED, "bin": -MISMATCHED, "dict": -UNSUPPORTED, "ts9": -UNSUPPORTED, "nope": -INVALID,
}
LONG = "ab" * 32       # 64 bytes


def hexs(s):
    return "S" + (s.encode().hex() or "-")


# the stripes of the set "m": (count, int key, string key); None: NULL
STRIPES = [
    [(1, 5, "x"), (2, None, ""), (3, 0, None), (4, 0, "")],
    [(10, 0, ""), (20, 7, LONG), (30, 5, "x"), (40, None, None)],
    [(100, 7, LONG), (200, -1, "ab"), (300, None, "")],
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_plan")
    exe, cases = str(d / "group_plan_check"), str(d / "cases.txt")
    with open(cases, "w") as f:
        for name in KEYS:
            f.write("keys one_%s flat %s\n" % (name, name))
        f.write("keys none flat\nkeys four flat i8 s b dec15_2\nkeys five flat i8 i16 i32 i64 s\nkeys twice flat s i64 s\nkeys null_name flat i64 -null-\n")
        f.write("keys q1 flat s vc\nkeys nested nested i64\nkeys second_bad flat i64 f64\n")
        for stripe in STRIPES:
            f.write("stripe m %d\n" % len(stripe))
            for count, i, s in stripe:
                f.write("g %d %s %s\n" % (count, "N" if i is None else "I%d" % i, "N" if s is None else hexs(s)))
        f.write("show m\nshow empty\n")
        f.write("cap at 65536\ncap over 65537\n")
        f.write("flags fine 0 256\nflags many 1 3\nflags count 0 257\nflags long_s 4 2\nflags long_i 2 2\nflags both 5 2\n")
        f.write("mask none -\nmask one 1\nmask ten 10\nmask all 32\nmask zero 0\nmask junk x\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "group_plan_check.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def keys(lines, name):
    """(status, [(kind, fkind, scale_or_unit)], message)"""
    ln = [x for x in lines if x.startswith("keys %s " % name)]
    assert len(ln) == 1, name
    head, msg = ln[0].split("\t")
    f = head.split()
    n = int(f[3])
    return int(f[2]), [tuple(int(x) for x in f[4 + 3 * k:7 + 3 * k]) for k in range(n)], msg


def test_every_key_kind(lines):
    for name, want in KEYS.items():
        st, got, msg = keys(lines, "one_%s" % name)
        if isinstance(want, int):
            assert st == -want and got == [] and "'%s'" % name in msg, (name, st, msg)
        else:
            assert (st, got) == (OK, [want]), (name, st, got, msg)


def test_key_counts_duplicates_and_nested(lines):
    assert keys(lines, "none")[0] == INVALID
    assert keys(lines, "four")[:2] == (OK, [KEYS["i8"], KEYS["s"], KEYS["b"], KEYS["dec15_2"]])
    st, _, msg = keys(lines, "five")
    assert st == INVALID and "4" in msg
    st, _, msg = keys(lines, "twice")
    assert st == INVALID and "'s'" in msg and "twice" in msg
    assert keys(lines, "null_name")[0] == INVALID
    assert keys(lines, "q1")[:2] == (OK, [KEYS["s"], KEYS["vc"]])
    st, _, msg = keys(lines, "nested")
    assert st == UNSUPPORTED and "'st'" in msg
    st, _, msg = keys(lines, "second_bad")
    assert st == MISMATCHED and "'f64'" in msg


def test_merge_of_stripes(lines):
    st = [x.split("\t")[0].split() for x in lines if x.startswith("stripe m ")]
    assert [(int(f[2]), int(f[3])) for f in st] == [(OK, 4), (OK, 6), (OK, 7)]
    # the model: a dict in first-appearance order
    want = {}
    for stripe in STRIPES:
        for count, i, s in stripe:
            want[(i, s)] = want.get((i, s), 0) + count
    assert len(want) == 7 and list(want)[:4] == [(5, "x"), (None, ""), (0, None), (0, "")]      # NULL, 0 and '' are three keys
    got = [x.split() for x in lines if x.startswith("group m ")]
    assert [int(g[2]) for g in got] == list(range(7))
    for g, ((i, s), count) in zip(got, want.items()):
        assert int(g[3]) == count, g
        assert g[4] == ("N:0:-1" if i is None else "I%d:0:-1" % i), g                       # kind I64, no unit
        assert g[5] == ("N:3:-1" if s is None else "%s:3:-1" % hexs(s)), g                  # kind STRING; the 64 bytes whole
    assert want[(7, LONG)] == 120 and want[(5, "x")] == 31 and want[(0, "")] == 14
    assert not [x for x in lines if x.startswith("group empty ")]


def test_total_cap(lines):
    cap = {x.split()[1]: x for x in lines if x.startswith("cap ")}
    assert cap["at"].split("\t")[0].split()[2:] == [str(OK), "65536"]
    head, msg = cap["over"].split("\t")
    assert head.split()[2] == str(UNSUPPORTED) and "65536" in msg


def test_flags_and_hash_mask(lines):
    fl = {x.split()[1]: (int(x.split("\t")[0].split()[2]), x.split("\t")[1]) for x in lines if x.startswith("flags ")}
    assert fl["fine"][0] == OK
    for name in ("many", "count", "both"):
        assert fl[name][0] == UNSUPPORTED and "256" in fl[name][1], name
    assert fl["long_s"][0] == UNSUPPORTED and "'s'" in fl["long_s"][1] and "64" in fl["long_s"][1]
    assert fl["long_i"][0] == UNSUPPORTED and "'i64'" in fl["long_i"][1]
    mask = {x.split()[1]: x.split()[2] for x in lines if x.startswith("mask ")}
    assert mask == {"none": "ffffffff", "one": "1", "ten": "3ff", "all": "ffffffff", "zero": "ffffffff", "junk": "ffffffff"}
