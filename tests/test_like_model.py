"""tests/like_model.py against the outside authority for the row filter's LIKE semantics, pyarrow.compute.match_like (which always
escapes with a backslash): every corner value against every corner pattern, nulls included."""
import pyarrow as pa
import pyarrow.compute as pc

import like_model as LM


def test_the_model_agrees_with_match_like():
    values = LM.VALUES + [None, None]
    arr = pa.array(values, pa.string())
    differing = 0
    for pattern in LM.PATTERNS:
        want = pc.match_like(arr, pattern).to_pylist()
        got = LM.like_column(values, pattern, "\\")
        assert got == want, (pattern, [(v, g, w) for v, g, w in zip(values, got, want) if g != w])
        differing += len({w for w in want if w is not None}) == 2
    assert differing >= len(LM.PATTERNS) - 3  # all but the keep-all patterns tell values apart


def test_the_corner_values_are_what_the_issue_names():
    lengths = sorted({len(v.encode()) for v in LM.long_values()})
    assert {31, 32, 33, 63, 64, 65, 300} <= set(lengths)
    for v in LM.long_values():
        b = v.encode()
        at = b.find(LM.NEEDLE.encode())
        assert at == 0 or at + 3 == len(b) or (at == 62 and len(b) >= 65) or "é" in v, v
    assert any(len(v.encode()) - len(v) == 3 for v in LM.VALUES)  # a 4-byte code point


def test_any_escape_character():
    for esc in LM.ESCAPES:
        other = [e for e in LM.ESCAPES if e != esc][0]
        assert LM.like("a%b", "a" + esc + "%b", esc) and not LM.like("axb", "a" + esc + "%b", esc)
        assert LM.like("a_b", "a" + esc + "_b", esc) and not LM.like("axb", "a" + esc + "_b", esc)
        assert LM.like("a" + esc + "b", "a" + esc + esc + "b", esc)
        assert LM.like("axb", "a" + esc + "xb", esc)  # any other byte behind the escape is itself
        assert LM.like("a" + other + "xb", "a" + other + "%b", esc)  # ... and another escape character is a character
    assert LM.like("a\\b", "a\\b") and LM.like("a\\%", "a\\%") and not LM.like("a%", "a\\%")  # without an escape a backslash is a byte
    assert LM.like(None, "%") is None and LM.like("a", None) is None
    for pattern, esc in LM.ESCAPED:
        back = pattern.replace("\\", "\\\\").replace(esc, "\\")
        arr = pa.array(LM.VALUES, pa.string())
        assert LM.like_column(LM.VALUES, pattern, esc) == pc.match_like(arr, back).to_pylist(), (pattern, esc)


def test_classification_and_the_pruning_rule():
    cases = {b"": "eq", b"abc": "eq", b"%": "all", b"%%%": "all", b"a%": "prefix", b"ab%%": "prefix", b"%a": "suffix", b"%ab%": "contains",
             b"_": "general", b"a_%": "general", b"a%b": "general", b"%a%b%": "general", b"a\\%": "eq", b"a\\": "invalid",
             b"a" * 1024: "eq", b"a" * 1025: "unsupported", b"\\a" * 1024: "eq", b"%".join([b"a"] * 64): "general",
             b"%".join([b"a"] * 65): "unsupported"}
    for pattern, want in cases.items():
        assert LM.classify(pattern, 0x5C) == want, pattern
    assert LM.classify(b"a\\", 0) == "eq" and LM.classify(b"a!%", 0x21) == "eq"
    assert LM.succ(b"ab") == b"ac" and LM.succ(b"a\xff") == b"b" and LM.succ(b"\xff\xff") is None
    assert LM.might_match(b"abc", b"abd", b"ab%") and not LM.might_match(b"b", b"c", b"ab%") and not LM.might_match(b"a", b"aa", b"ab%")
    assert LM.might_match(b"a", b"z", b"%b") and LM.might_match(b"zz", b"zzz", b"\xff\xff%") is False
    assert LM.might_match(b"\xff\xff\x01", b"\xff\xff\x02", b"\xff\xff_")
