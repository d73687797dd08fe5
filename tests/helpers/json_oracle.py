"""An independent oracle for the JSON parse and count kernels: ``json.loads`` and the documented
"simple row" rule, in plain Python.  Nothing here calls the package.

* ``numbers``       what the reference's ``json.loads(record.value)`` gives for a flat numeric array;
* ``simple_count``  the documented pre-scan rule (json_text.cpp, span.h): which rows the device parses;
* ``guess``         the width a row that is left to the host gets before its host parse;
* ``expected``      values / lengths / mask of a batch, through f64 -> f32 -> dtype as known_records does;
* ``sweep_tokens``  every token of 1..4 characters over ``019.-`` (780), ``sweep_rows`` their two framings.
"""
import itertools
import json

import torch

from helpers.known_records import expected_varlen

WS = b" \t\n\r"
NUMBER_CHARS = b"0123456789.-"
MAX_SIMPLE_TOKEN = 16
SWEEP_ALPHABET = "019.-"


def numbers(text: bytes):
    """``[float(x), ...]`` when ``json.loads`` gives a flat list of int / float (bool does not
    count), else ``None``."""
    try:
        v = json.loads(text)
    except ValueError:  # JSONDecodeError and UnicodeDecodeError
        return None
    if not isinstance(v, list) or not all(type(x) in (int, float) for x in v):
        return None
    return [float(x) for x in v]


def _frame(text: bytes):
    """The interior of ``[`` ... ``]`` after trimming whitespace, or ``None``."""
    t = text.strip(WS)
    if len(t) < 2 or t[:1] != b"[" or t[-1:] != b"]":
        return None
    return t[1:-1]


def simple_count(text: bytes) -> int:
    """Element count of a "simple" row (commas + 1, 0 for a blank interior), or -1."""
    body = _frame(text)
    if body is None:
        return -1
    run = commas = 0
    any_tok = False
    for c in body:
        if c in NUMBER_CHARS:
            any_tok = True
            run += 1
            if run > MAX_SIMPLE_TOKEN:
                return -1
        else:
            run = 0
            if c == ord(","):
                commas += 1
            elif c not in WS:
                return -1
    if not any_tok:
        return 0 if commas == 0 else -1
    return commas + 1


def guess(text: bytes) -> int:
    """commas + 1 of a framed text whose interior is not blank, else 0."""
    body = _frame(text)
    if body is None or not body.strip(WS):
        return 0
    return body.count(b",") + 1


def expected(rows, dtype: torch.dtype, L: int, pad=0.0, trunc=None):
    """(values [n, L], lengths, mask) of rows given as lists of Python floats (``numbers``)."""
    t = [torch.tensor(r, dtype=torch.float64).to(torch.float32) for r in rows]
    return expected_varlen(t, dtype, L, pad, trunc)


def sweep_tokens():
    """Every token of 1 to 4 characters over ``019.-``."""
    return ["".join(p) for n in range(1, 5) for p in itertools.product(SWEEP_ALPHABET, repeat=n)]


def sweep_rows():
    """[(row text, token)]: each sweep token as ``[tok]`` and as ``[7, tok ]``."""
    out = []
    for tok in sweep_tokens():
        out.append((("[" + tok + "]").encode(), tok))
        out.append((("[7, " + tok + " ]").encode(), tok))
    return out


def ws_run(n: int, seed: int = 0) -> bytes:
    """``n`` whitespace characters, every kind in turn."""
    return bytes(WS[(seed + i) % 4] for i in range(n))


def count_corpus():
    """The rows of the device-count tests (and of the CPU scan agreement): text shorter than the
    framing, blank and empty arrays, whitespace around the framing at the 16-byte chunk and 64-lane
    search edges, bytes outside the alphabet, runs of 16 / 17 number characters across the 1 KiB
    pass and the 2 KiB window, rows of exactly one pass, and the token-sweep rejects."""
    rows = [b"", b"[", b"]", b"5", b" ", b" \t\n\r  ", ws_run(70), b"[]", b"[ ]", b"[,]", b"[ , ]", b"[1,]",
            b"[1, 2.5, -3]", b"[-0, -0.0, 0.5]", b"[" + ws_run(40) + b"]", b"[" + ws_run(40) + b",]"]
    for n in (0, 1, 15, 16, 63, 64, 65, 130):
        rows.append(ws_run(n) + b"[1.5, -2,3 ]")
        rows.append(b"[4 ,5.25]" + ws_run(n, 1))
        rows.append(ws_run(n, 2) + b"[-6,7,8.125]" + ws_run(n, 3))
        rows.append(ws_run(n) + b"[1, 2" + ws_run(n, 1))     # no closing bracket behind the trim
        rows.append(ws_run(n) + b"[]" + ws_run(n))
    for c in (b"e", b"N", b'"', b"/", b"+", b"\xc3", b"\x80", b"[", b"]", b"\0"):
        rows.append(b"[1" + c + b"5]")
        rows.append(b"[1, " + c + b", 2]")
        rows.append(b"[" + b"3," * 700 + b"1" + c + b"2]")  # past the first 1 KiB pass
    rows += [b"[1e5]", b"[NaN]", b"[-Infinity, 2]", b"[1, [2]]", b'["1"]', b"{}", b"[true]", b"[null]", b"[1 2]",
             b"[1,,2]"]
    d16, d17 = b"1234567890123.25", b"12345678901234.25"
    assert len(d16) == 16 and len(d17) == 17
    for edge in (1024, 2048):
        for off in range(edge - 17, edge + 2):
            # "[" + k * "1," + spaces so that the run's first character sits at byte `off`
            head = b"[" + b"1," * ((off - 1) // 2 - 3)
            head += b" " * (off - len(head))
            rows.append(head + d16 + b",8]")
            rows.append(head + d17 + b",8]")
            if off % 3 == 0:  # behind whitespace: the framing search, every offset one further
                rows.append(b"\n" + head + d16 + b",8] ")
                rows.append(b"\n" + head + d17 + b",8] ")
    for n in (32, 33):
        rows.append(b"[" + b"7" * n + b"]")
        rows.append(b"[1, " + b"7" * n + b", 2]")
    for T in (1024, 1025):
        body = b"[" + b"2," * 400
        rows.append(body + b" " * (T - len(body) - 2) + b"9]")
    rows += [r for r, _ in sweep_rows() if numbers(r) is None]
    return rows
