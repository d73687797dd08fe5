"""The host JSON parser and pre-scan against an oracle that makes no call into the package
(tests/helpers/json_oracle.py: ``json.loads`` and the documented "simple row" rule).

The reference decodes a record with ``json.loads(record.value)``: a row it rejects must raise here
too, and a row it accepts must give the same float32 bits.  The sweep covers every token of 1 to 4
characters over ``019.-`` -- leading zeros (``01``, ``-00``), an empty integer part (``.5``), lone
signs and dots -- in two framings.
"""
import numpy as np
import pytest
import torch

from helpers import json_oracle as jo
from torchkafka_amd.ops.native import core


def test_sweep_has_both_verdicts():
    verdicts = [jo.numbers(("[" + t + "]").encode()) is not None for t in jo.sweep_tokens()]
    assert len(verdicts) == 780
    assert sum(verdicts) >= 150 and len(verdicts) - sum(verdicts) >= 600  # 171 and 609
    for text, tok in jo.sweep_rows():  # both framings of a token get the same verdict
        assert (jo.numbers(text) is None) == (jo.numbers(("[" + tok + "]").encode()) is None)


def test_parse_accepts_exactly_what_json_loads_accepts():
    c = core()
    wrongly_accepted, wrongly_rejected = [], []
    for text, _tok in jo.sweep_rows():
        want = jo.numbers(text)
        try:
            got = c.parse_json_f32(text)
        except ValueError:
            got = None
        if want is None:
            if got is not None:
                wrongly_accepted.append(text)
            continue
        if got is None:
            wrongly_rejected.append(text)
            continue
        exp = torch.tensor(want, dtype=torch.float64).to(torch.float32).numpy()
        assert np.array_equal(np.asarray(got, dtype=np.float32).view(np.int32), exp.view(np.int32)), text
    assert not wrongly_rejected, wrongly_rejected[:20]
    assert not wrongly_accepted, (len(wrongly_accepted), wrongly_accepted[:20])


@pytest.mark.parametrize("text", [b"[01]", b"[00]", b"[-00]", b"[.5]", b"[-.5]", b"[-01.5]", b"[007, 1]", b"[1, 00.5]",
                                  b"[0123456789012345]", b"[01e2]", b"[.5e1]", b"[-]", b"[-e5]"])
def test_leading_zeros_and_empty_integer_part_raise(text):
    assert jo.numbers(text) is None
    with pytest.raises(ValueError):
        core().parse_json_f32(text)


@pytest.mark.parametrize("text", [b"[0]", b"[-0]", b"[-0.0]", b"[0.5]", b"[-0.5e1]", b"[0e5]", b"[10, 100.001]",
                                  b"[0.000, -0.000]", b"[0E-3]"])
def test_zero_forms_of_json_still_parse(text):
    want = torch.tensor(jo.numbers(text), dtype=torch.float64).to(torch.float32).numpy()
    got = np.asarray(core().parse_json_f32(text), dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("simd", [True, False])
def test_scan_matches_the_documented_rule_over_the_count_corpus(simd):
    c = core()
    rows = jo.count_corpus()
    assert len(rows) > 1000
    counts = [jo.simple_count(t) for t in rows]
    assert sum(k >= 0 for k in counts) > 100 and sum(k < 0 for k in counts) > 100
    for t, want in zip(rows, counts):
        assert c.json_scan_simple(t, simd) == want, t[:80] + b"..." + t[-40:]
