"""An independent model of the row filter's LIKE (include/orcgpu.h, ORCGPU_PRED_LIKE) in plain Python: the pattern is translated to
a regular expression over str -- `%` -> `.*`, `_` -> `.` (one code point, a newline included: re.DOTALL), the escape character
makes the next character a literal -- and the WHOLE value must match.  Any escape character is supported.  Also: what the plan
compiler is to make of a pattern (classify) and the row-group pruning rule (might_match), as the issue states them."""
import re

ESCAPES = ("\\", "!", "#")
LIKE_MAX_BYTES, LIKE_MAX_PARTS = 1024, 64


def elements(pattern, escape=None):
    """-> list of ("lit", ch) / ("one",) / ("any",); ValueError when the pattern ends in the escape."""
    out, k = [], 0
    while k < len(pattern):
        ch = pattern[k]
        if escape is not None and ch == escape:
            if k + 1 == len(pattern):
                raise ValueError("the pattern ends in its escape")
            out.append(("lit", pattern[k + 1]))
            k += 2
            continue
        out.append(("any",) if ch == "%" else ("one",) if ch == "_" else ("lit", ch))
        k += 1
    return out


def compile_like(pattern, escape=None):
    rx = "".join(".*" if e[0] == "any" else "." if e[0] == "one" else re.escape(e[1]) for e in elements(pattern, escape))
    return re.compile(rx, re.DOTALL)


def like(value, pattern, escape=None):
    """True / False, or None (UNKNOWN) when the value or the pattern is None."""
    if value is None or pattern is None:
        return None
    return compile_like(pattern, escape).fullmatch(value) is not None


def like_column(values, pattern, escape=None):
    if pattern is None:
        return [None] * len(values)
    rx = compile_like(pattern, escape)
    return [None if v is None else rx.fullmatch(v) is not None for v in values]


def classify(pattern, escape=None):
    """What the plan compiler makes of a pattern given as BYTES (escape: an int, 0 = none): one of "invalid" (trailing escape),
    "unsupported" (the limits), "eq", "all", "prefix", "suffix", "contains", "general"."""
    els, k = [], 0
    while k < len(pattern):
        b = pattern[k]
        if escape and b == escape:
            if k + 1 == len(pattern):
                return "invalid"
            els.append("l")
            k += 2
            continue
        els.append("%" if b == 0x25 else "_" if b == 0x5F else "l")
        k += 1
    if len(els) > LIKE_MAX_BYTES:
        return "unsupported"
    s = "".join(els)
    if "%" not in s and "_" not in s:
        return "eq"
    parts = [p for p in s.split("%") if p]
    if len(parts) > LIKE_MAX_PARTS:
        return "unsupported"
    if not parts:
        return "all"
    if len(parts) == 1 and "_" not in parts[0]:
        start, end = not s.startswith("%"), not s.endswith("%")
        if start != end:
            return "prefix" if start else "suffix"
        if not start:
            return "contains"
    return "general"


def literal_prefix(pattern, escape=0):
    """(the bytes in front of the first unescaped wildcard, whether the pattern holds a wildcard at all); None: trailing escape"""
    out, k = bytearray(), 0
    while k < len(pattern):
        b = pattern[k]
        if escape and b == escape:
            if k + 1 == len(pattern):
                return None
            out.append(pattern[k + 1])
            k += 2
            continue
        if b in (0x25, 0x5F):
            return bytes(out), True
        out.append(b)
        k += 1
    return bytes(out), False


def succ(p):
    """p with its last byte that is not 0xFF incremented and everything behind it cut off; None when p is all 0xFF"""
    p = bytes(p).rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def might_match(lower, upper, pattern, escape=0):
    """The pruning rule for a pattern with a wildcard on a group with the String bounds [lower, upper] (bytes)."""
    got = literal_prefix(pattern, escape)
    if got is None or not got[1] or not got[0]:
        return True
    p = got[0]
    s = succ(p)
    return upper >= p and (s is None or lower < s)


# ---- the corner cases the tests share ----
NEEDLE = "aab"


def long_values():
    """values of 31 .. 300 BYTES with NEEDLE at the very start, at the very end and (where the value is long enough) over byte 64"""
    out = []
    for n in (31, 32, 33, 63, 64, 65, 300):
        fill = "c" * (n - len(NEEDLE))
        out += [NEEDLE + fill, fill + NEEDLE]
        if n >= 65:
            out.append("c" * 62 + NEEDLE + "c" * (n - 62 - len(NEEDLE)))  # bytes 62, 63 | 64
        if n == 65:
            out.append("c" * 61 + "é" + NEEDLE[1:] + "c")  # ... and a two-byte character over the edge of a short value
    return out


VALUES = ["", "a", "aba", "abba", "aaab", "ab\nba", "héllo", "hé", "a\U0001F600b", "a%b", "a_b", "a\\b"] + long_values()
PATTERNS = ["", "%", "%%", "_", "__", "%_%", "a%", "%a", "%aab", "ab%ba", "%a%a%", "h_llo", "h_", "_é", "a\\%b", "a\\_b", "a\\\\b", "%\n%",
            "a%b%a", "%a%b%a%b%a%", "%" + NEEDLE + "%", NEEDLE + "%", "_\U0001F600%", "%c_" + NEEDLE[1:] + "c"]
KEEP_ALL = ("%", "%%")
# (pattern, escape) beyond the backslash
ESCAPED = [("a!%b", "!"), ("a#_b", "#"), ("%!_%", "!"), ("a!\\b", "!")]
