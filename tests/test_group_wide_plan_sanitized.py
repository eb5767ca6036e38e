"""The host side of GROUP BY's limits and wide path under AddressSanitizer + UBSan on the CPU: tests/hostcheck/group_wide_check.cpp
compiles orc_rust_amd/csrc/orcgpu_group_plan.inc -- the text liborcgpu.so is built from -- into a stand-alone program.  The limit
checks; which path a limit takes, its table's slots and its sort's passes; the wide workspace's layout; the merge of stripes of a
thousand groups against a dict, with the refusal at exactly max_total + 1; the flags check against the limit that was set.
No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, UNSUPPORTED, INVALID = 0, 7, 101
ALIGN = 256
LIMITS = (256, 257, 65536, 65537, 2 ** 20)
N_IN = (0, 1, 63, 64, 65, 2 ** 20 + 1)
INSNS = (1, 64)
LAYOUT_LIMIT, LAYOUT_KEYS, LAYOUT_BASE = 2 ** 20, 3, 1000
STRIPES, PER, STEP = 3, 1000, 500          # three stripes of 1000 groups, each sharing 500 with the one before: 2000 groups


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_wide")
    exe, cases = str(d / "group_wide_check"), str(d / "cases.txt")
    with open(cases, "w") as f:
        f.write("limits default 0 0\nlimits one 1 1\nlimits top 1048576 16777216\nlimits groups_over 1048577 0\nlimits total_over 0 16777217\n")
        f.write("limits total_below 300 299\nlimits default_total_below 65537 0\nlimits total_below_default 0 255\nlimits wide 300 0\n")
        for limit in LIMITS + (1, 2, 300, 70000):
            f.write("plan %d\n" % limit)
        for n_in in N_IN:
            for n_insn in INSNS:
                f.write("layout %d %d %d %d %d\n" % (LAYOUT_LIMIT, n_in, n_insn, LAYOUT_KEYS, LAYOUT_BASE))
        f.write("layout 300 5000 4 1 0\n")
        f.write("merge at %d %d %d %d\nmerge under %d %d %d %d\n" % (2000, STRIPES, PER, STEP, 1999, STRIPES, PER, STEP))
        f.write("flags fine 300 0 300\nflags count 300 0 301\nflags many 300 1 5\nflags narrow 100 0 101\nflags long_k 300 2 5\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "group_wide_check.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def test_limits(lines):
    got = {}
    for x in lines:
        if x.startswith("limits "):
            head, msg = x.split("\t")
            f = head.split()
            got[f[1]] = (int(f[2]), int(f[3]), int(f[4]), msg)
    assert got["default"][:3] == (OK, 256, 65536) and got["one"][:3] == (OK, 1, 1) and got["top"][:3] == (OK, 2 ** 20, 2 ** 24)
    assert got["wide"][:3] == (OK, 300, 65536)
    assert got["groups_over"][0] == INVALID and "1048577" in got["groups_over"][3]
    assert got["total_over"][0] == INVALID and "16777217" in got["total_over"][3]
    for name, a, b in (("total_below", "299", "300"), ("default_total_below", "65536", "65537"), ("total_below_default", "255", "256")):
        assert got[name][0] == INVALID and a in got[name][3] and b in got[name][3], name


def test_path_slots_and_passes(lines):
    plan = {int(x.split()[1]): tuple(int(v) for v in x.split()[2:]) for x in lines if x.startswith("plan ")}
    # (wide, slots, passes): slots the power of two >= 4 x the limit; a pass per 8 bits of the group numbers 0 .. limit - 1
    assert plan[256] == (0, 1024, 1)
    assert plan[257] == (1, 2048, 2)
    assert plan[65536] == (1, 2 ** 18, 2)
    assert plan[65537] == (1, 2 ** 19, 3)
    assert plan[2 ** 20] == (1, 2 ** 22, 3)
    assert plan[300] == (1, 2048, 2) and plan[70000] == (1, 2 ** 19, 3)
    assert plan[1][0] == 0 and plan[2][0] == 0
    for limit, (_, slots, passes) in plan.items():
        assert slots & (slots - 1) == 0 and slots >= 4 * limit and (slots // 2 < 4 * limit or slots == 4)
        assert 2 ** (8 * passes) >= limit and (passes == 1 or 2 ** (8 * (passes - 1)) < limit)


def layouts(lines):
    for x in lines:
        if x.startswith("layout "):
            f = x.split()
            head = [int(v) for v in f[1:10]]
            parts = [(p.split(":")[0], int(p.split(":")[1]), int(p.split(":")[2])) for p in f[10:]]
            yield head, parts


def test_workspace_layout(lines):
    seen = set()
    for (limit, n_in, n_insn, n_keys, slots, passes, tiles, cap, total), parts in layouts(lines):
        seen.add((limit, n_in, n_insn))
        base = LAYOUT_BASE if limit == LAYOUT_LIMIT else 0
        assert tiles == max(1, -(-n_in // 2048)) and cap == min(limit, n_in)
        at = base
        for name, off, size in parts:           # aligned, in order, none overlapping
            assert off % ALIGN == 0 and off >= at, (name, off, at)
            assert off - at < ALIGN, (name, "a gap of more than the alignment")
            at = off + size
        assert at <= total < at + ALIGN and total % ALIGN == 0
        size = {name: s for name, _, s in parts}
        padded = -(-n_in // 64) * 64
        assert size["table"] == slots * 16 and size["slot_group"] == slots * 4 and size["ctl"] == 16
        assert size["plane"] == size["keys0"] == size["keys1"] == size["rows0"] == size["rows1"] == padded * 4
        assert size["hist"] == tiles * 1024 and size["blk_first"] == size["blk_kept"] == tiles * 4
        assert size["seg"] == cap * 4 and size["key_recs"] == cap * n_keys * 88 and size["vals"] == cap * n_insn * 48     # by the rows, not by the limit
    assert seen == {(LAYOUT_LIMIT, n, i) for n in N_IN for i in INSNS} | {(300, 5000, 4)}


def test_merge_against_a_dict(lines):
    want = {}
    for s in range(STRIPES):
        for g in range(PER):
            k = s * STEP + g
            total, rows = want.get(k, (0, 0))
            want[k] = (total + k + s, rows + 1)
    assert len(want) == 2000
    head = {x.split()[1]: x for x in lines if x.startswith("merge ")}
    assert head["at"].split("\t")[0].split()[2:] == [str(OK), "2000"]                 # exactly max_total groups: accepted
    got = [tuple(int(v) for v in x.split()[2:]) for x in lines if x.startswith("mgroup at ")]
    assert got == [(i, k, v[0], v[1]) for i, (k, v) in enumerate(want.items())]       # first-appearance order, the sums, the rows
    h, msg = head["under"].split("\t")
    assert h.split()[2] == str(UNSUPPORTED) and "1999" in msg                           # max_total + 1 groups: refused, the limit in the message
    assert not [x for x in lines if x.startswith("mgroup under ")]


def test_flags_against_the_limit_that_was_set(lines):
    fl = {x.split()[1]: (int(x.split("\t")[0].split()[2]), x.split("\t")[1]) for x in lines if x.startswith("flags ")}
    assert fl["fine"][0] == OK
    for name in ("count", "many"):
        assert fl[name][0] == UNSUPPORTED and "300" in fl[name][1], name
    assert fl["narrow"][0] == UNSUPPORTED and "100" in fl["narrow"][1]              # a limit below 256 holds on the narrow path too
    assert fl["long_k"][0] == UNSUPPORTED and "'k'" in fl["long_k"][1]
