"""LIKE patterns through the row filter's plan compiler under AddressSanitizer + UBSan on the CPU:
tests/hostcheck/filter_plan_like_check.cpp compiles orc_rust_amd/csrc/orcgpu_filter_plan.inc and orcgpu_like.inc -- the text
liborcgpu.so is built from -- into a stand-alone program that prints what became of every pattern; here every line is compared
with what tests/like_model.py says the pattern is.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

import like_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
FOP_CMP_STRING, FOP_UNKNOWN, FOP_NOT, FOP_LIKE = 3, 7, 12, 13


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_plan_like") / "filter_plan_like_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_plan_like_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def expected_parts(pattern, escape):
    """the model's own cut of the pattern, in the program's notation"""
    els, k = [], 0
    while k < len(pattern):
        b = pattern[k]
        if escape and b == escape:
            els.append("%02x" % pattern[k + 1])
            k += 2
            continue
        els.append("%" if b == 0x25 else "__" if b == 0x5F else "%02x" % b)
        k += 1
    if "%" not in els and "__" not in els:
        return "=" + "".join(els)
    parts, cur = [], []
    for e in els:
        if e == "%":
            if cur:
                parts.append("".join(cur))
            cur = []
        else:
            cur.append(e)
    if cur:
        parts.append("".join(cur))
    if not parts:
        return "-"
    return ("-" if els[0] == "%" else "S") + "|".join(parts) + ("-" if els[-1] == "%" else "E")


def test_every_pattern_is_what_the_model_says(lines):
    seen = {}
    pats = [ln for ln in lines if ln[0] == "pat"]
    assert len(pats) > 3000
    for _, hx, escape, rc, cls, parts in pats:
        pattern, escape, rc = (b"" if hx == "-" else bytes.fromhex(hx)), int(escape), int(rc)
        want = LM.classify(pattern, escape)
        seen[want] = seen.get(want, 0) + 1
        if want == "invalid":
            assert (rc, cls) == (INVALID, "-"), (pattern, escape)
        elif want == "unsupported":
            assert (rc, cls) == (UNSUPPORTED, "-"), (pattern, escape)
        else:
            assert (rc, cls) == (OK, want), (pattern, escape, cls)
            assert parts == expected_parts(pattern, escape), (pattern, escape)
    assert all(seen.get(c, 0) >= 20 for c in ("eq", "all", "prefix", "suffix", "contains", "general", "invalid")), seen
    assert seen["unsupported"] >= 6, seen


def test_the_corner_patterns_and_the_limits(lines):
    got = {(ln[1], int(ln[2])): (int(ln[3]), ln[4]) for ln in lines if ln[0] == "pat"}
    for p in LM.PATTERNS + [p for p, _ in LM.ESCAPED]:
        key = p.encode().hex() or "-"
        for escape in (0x5C, 0x21, 0):
            assert (key, escape) in got, (p, escape)
    b = 0x5C
    assert got[((b"a" * 1024).hex(), b)] == (OK, "eq") and got[((b"a" * 1025).hex(), b)] == (UNSUPPORTED, "-")
    assert got[((b"a" * 1023 + b"%").hex(), b)] == (OK, "prefix") and got[((b"a" * 1024 + b"%").hex(), b)] == (UNSUPPORTED, "-")
    assert got[((b"%" * 1024).hex(), b)] == (OK, "all") and got[((b"_" * 1025).hex(), b)] == (UNSUPPORTED, "-")
    assert got[((b"\\%" * 1024).hex(), b)] == (OK, "eq") and got[((b"\\%" * 1024 + b"x").hex(), b)] == (UNSUPPORTED, "-")
    p64 = b"a" + b"%b" * 63
    assert got[(p64.hex(), b)] == (OK, "general") and got[((p64 + b"%c").hex(), b)] == (UNSUPPORTED, "-")
    assert got[((b"%" + p64 + b"%").hex(), b)] == (OK, "general") and got[((b"%" + p64 + b"%c%").hex(), b)] == (UNSUPPORTED, "-")
    assert got[((b"a" * 5000).hex(), b)] == (UNSUPPORTED, "-")
    assert got[(b"a\\".hex(), b)] == (INVALID, "-") and got[(b"a\\".hex(), 0)] == (OK, "eq")


def test_refusals_name_the_column(lines):
    bad = {ln[1]: tuple(int(x) for x in ln[2:]) for ln in lines if ln[0] == "bad"}
    assert bad["trailing_escape"][:2] == (INVALID, 1)
    for name in ("escape_200", "escape_negative", "escape_128", "length_without_bytes"):
        assert bad[name][:2] == (INVALID, 1), name
    for name in ("binary_column", "int_column", "int64_literal", "null_pattern_on_int"):
        assert bad[name][:2] == (MISMATCHED, 1), name
    assert bad["null_pattern"] == (OK, 0, 1, FOP_UNKNOWN)
    assert bad["no_such_column"][:2] == (INVALID, 1) and bad["no_column_name"][0] == INVALID
    tree = [ln for ln in lines if ln[0] == "tree"][0]
    assert [int(x) for x in tree[2:]] == [OK, 2, FOP_LIKE]  # LIKE, NOT (an AND of one child emits nothing)
    planes = [ln for ln in lines if ln[0] == "planes"][0]
    assert [int(x) for x in planes[1:]] == [0, 0, 1]  # plane 0, the keep-all shape without one, plane 1
