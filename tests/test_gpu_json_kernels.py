"""json_rows_kernel, json_count_kernel and the fused count at the kernel level, against an oracle
that makes no call into the package (tests/helpers/json_oracle.py: ``json.loads``, the documented
"simple row" rule, f64 -> f32 -> dtype casts in plain torch).  Every comparison is bit-exact.

Host-framed path (``launch_json_rows``; the descriptors carry the oracle's counts): the token
grammar, rounding at every destination dtype's ties, the 2 KiB window and token-table edges.
Device counting (``launch_json_group`` after ``json_count_kernel``) and fused counting (the parse
block counts its own row): one corpus of framing, alphabet, run-length and pass / window edges, run
through both, with and without truncation.
"""
import random

import numpy as np
import pytest
import torch

from helpers import json_oracle as jo
from helpers.known_records import (assert_same, bf16_tie_values, e4m3_tie_values, f16_tie_values, special_values)

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float8_e4m3fn: 3}
ERR_TAG = 1 << 30  # tk::kSpanParseErrBit: what the driver's group launches pass
CTR_TAG = 5
_CACHE = {}


def _up(x, a):
    return (x + a - 1) // a * a


def _esize(dt):
    return torch.empty((), dtype=dt).element_size()


# ----------------------------------------------------------------------------- launches
def run_rows(texts, dtype, L, pad=0.0):
    """One ``launch_json_rows`` over simple rows framed with the oracle's counts (32-byte aligned
    text, as the worker frames it).  -> (out [n, L], lengths, mask, err word)."""
    from torchkafka_amd.ops.native import hip

    desc = np.zeros((len(texts), 4), dtype=np.int32)
    vals = bytearray()
    for i, t in enumerate(texts):
        cnt = jo.simple_count(t)
        assert cnt >= 0, t[:60]
        at = _up(len(vals), 32)
        vals.extend(b"\0" * (at - len(vals)))
        vals.extend(t)
        desc[i] = (at, len(t), cnt, cnt)
    vals.extend(b"\0" * (64 - len(vals) % 16))  # the kernel reads whole 16-byte chunks
    d_desc = torch.from_numpy(desc).cuda()
    d_vals = torch.frombuffer(vals, dtype=torch.uint8).cuda()
    out = torch.full((len(texts), L), 7, dtype=torch.float32, device="cuda").to(dtype)
    lengths = torch.full((len(texts),), -1, dtype=torch.int64, device="cuda")
    mask = torch.full((len(texts), L), 3, dtype=torch.uint8, device="cuda")
    err = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hip().launch_json_rows(d_desc.data_ptr(), d_vals.data_ptr(), out.data_ptr(), DT[dtype], len(texts), L, pad,
                           lengths.data_ptr(), mask.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu(), lengths.cpu(), mask.cpu(), int(err.item())


def check_rows(texts, dtype, L=None, pad=0.0):
    """Runs ``texts`` (all valid and simple) in one launch and compares with the oracle."""
    nums = [jo.numbers(t) for t in texts]
    assert all(v is not None for v in nums)
    L = max(len(v) for v in nums) if L is None else L
    out, lengths, mask, err = run_rows(texts, dtype, L, pad)
    exp, elen, emask = jo.expected(nums, dtype, L, pad)
    assert err == -1
    assert torch.equal(lengths, elen)
    assert torch.equal(mask, emask.to(torch.uint8))
    assert_same(out, exp, "json_rows_kernel")


def run_group(batches, dtype, L, mode, mult=1, trunc=-1, pad=0.0, err_tag=ERR_TAG, cap_cut=None):
    """``batches`` (lists of row texts) through ``launch_json_group``, ``JSON_MAX_GROUP`` batches a
    launch, all launches queued before one synchronize.  ``mode``: "host" (descriptors with the
    oracle's counts, no count words), "count" (json_count_kernel first) or "fused".  Texts are
    staged 16-byte aligned, each batch's area 256-byte aligned with ``vals_cap`` its exact size
    (``cap_cut`` = {batch: bytes}: a smaller cap, the text beyond it still there).  ``L`` is the
    capacity of every batch's output.  -> dict of CPU tensors."""
    from torchkafka_amd.ops.native import hip

    h = hip()
    nb = len(batches)
    row0 = np.cumsum([0] + [len(b) for b in batches])
    total = int(row0[-1])
    desc = np.zeros((total, 4), dtype=np.int32)
    vals = bytearray()
    area, cap = [], []
    for b, rows in enumerate(batches):
        start = _up(len(vals), 256)
        vals.extend(b"\0" * (start - len(vals)))
        for i, t in enumerate(rows):
            off = _up(len(vals) - start, 16)
            vals.extend(b"\0" * (start + off - len(vals)))
            vals.extend(t)
            if mode == "host":
                cnt = jo.simple_count(t)
                assert cnt >= 0
                desc[row0[b] + i] = (off, len(t), cnt, cnt if trunc < 0 else min(cnt, trunc))
            else:  # as json_stage_kernel leaves a device-counted row
                desc[row0[b] + i] = (off, len(t), h.JSON_COUNT_ON_DEVICE, 0)
        vals.extend(b"\0" * (_up(len(vals) - start, 16) - (len(vals) - start)))
        area.append(start)
        cap.append(len(vals) - start if cap_cut is None or b not in cap_cut else cap_cut[b])
    vals.extend(b"\0" * 256)
    es = _esize(dtype)
    d_desc = torch.from_numpy(desc).cuda()
    d_vals = torch.frombuffer(vals, dtype=torch.uint8).cuda()
    out = torch.full((total * L,), 7, dtype=torch.float32, device="cuda").to(dtype)
    lengths = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    mask = torch.full((total * L,), 3, dtype=torch.uint8, device="cuda")
    err = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    ctr = torch.zeros((nb, 2), dtype=torch.int64, device="cuda")
    info = torch.tensor([[-7, 0, -7]] * nb, dtype=torch.int32, device="cuda")
    dev = mode != "host"
    stream = torch.cuda.current_stream().cuda_stream
    G = h.JSON_MAX_GROUP
    for g0 in range(0, nb, G):
        ks = range(g0, min(nb, g0 + G))
        h.launch_json_group(
            desc=[d_desc.data_ptr() + 16 * int(row0[k]) for k in ks],
            values=[d_vals.data_ptr() + area[k] for k in ks],
            vals_cap=[cap[k] for k in ks],
            out=[out.data_ptr() + int(row0[k]) * L * es for k in ks],
            L=[L] * len(ks), n_rows=[len(batches[k]) for k in ks],
            lengths=[lengths.data_ptr() + 8 * int(row0[k]) for k in ks],
            mask=[mask.data_ptr() + int(row0[k]) * L for k in ks],
            err=[err.data_ptr() + 4 * k for k in ks],
            ctr=[ctr.data_ptr() + 16 * k if dev else 0 for k in ks],
            ctr_tag=[CTR_TAG] * len(ks), trunc=[trunc] * len(ks),
            info=[info.data_ptr() + 12 * k if dev else 0 for k in ks],
            dst_dtype=DT[dtype], pad=pad, mult=mult, err_tag=err_tag, fused_count=mode == "fused",
            count_first=mode == "count", stream=stream)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "lengths": lengths.cpu(), "mask": mask.cpu(), "err": err.cpu(), "ctr": ctr.cpu(),
            "info": info.cpu(), "desc": d_desc.cpu(), "row0": row0}


# ----------------------------------------------------------------------------- E: host-framed path
def test_token_sweep_accepted_rows_are_bit_exact():
    rows = [t for t, _ in jo.sweep_rows() if jo.numbers(t) is not None]
    assert len(rows) >= 300
    check_rows(rows, torch.float32)


def test_token_sweep_rejected_rows_are_flagged():
    """Each row json.loads rejects, in a two-row batch of its own: its batch's err word names row 1
    and the good row before it still parses."""
    bad = [t for t, _ in jo.sweep_rows() if jo.numbers(t) is None]
    assert len(bad) >= 1200
    res = run_group([[b"[1]", t] for t in bad], torch.float32, L=2, mode="host", err_tag=0, pad=-3.0)
    out = res["out"].view(len(bad), 2, 2)
    not_flagged = [bad[i] for i in (res["err"] != 1).nonzero().flatten().tolist()]
    assert not not_flagged, (len(not_flagged), not_flagged[:20])
    assert torch.equal(out[:, 0, :], torch.tensor([1.0, -3.0]).expand(len(bad), 2))
    assert torch.equal(res["lengths"].view(len(bad), 2)[:, 0], torch.ones(len(bad), dtype=torch.int64))


def _short_reprs(values, at_least):
    """repr(float) of the finite f32 ``values`` that has no exponent and at most 16 characters."""
    toks = []
    for x in values.to(torch.float64).tolist():
        r = repr(x)
        if "e" not in r and "n" not in r and len(r) <= 16:  # "n": inf / nan
            toks.append(r)
    assert len(toks) >= at_least, len(toks)
    return toks


def _edge_tokens():
    if "edge" not in _CACHE:
        toks = (_short_reprs(bf16_tie_values(), 3900) + _short_reprs(f16_tie_values(), 10000) +
                _short_reprs(e4m3_tie_values(), 500) + _short_reprs(special_values(), 20))
        toks += [str(v) for v in range(2 ** 53 - 2, 2 ** 53 + 4)]
        toks += [str(2 ** 24 + 1), str(2 ** 24 + 3), "9999999999999999", "0.00000000000001", "-99999999999.999"]
        rnd = random.Random(2024)

        def digits(n, first_nonzero):
            s = "".join(rnd.choice("0123456789") for _ in range(n))
            return (rnd.choice("123456789") + s[1:]) if first_nonzero and n > 1 else s

        for _ in range(256):
            k = rnd.randint(1, 14)
            toks.append(digits(16, True))
            toks.append("-" + digits(15, True))
            toks.append(digits(k, True) + "." + digits(15 - k, False))
            k = rnd.randint(1, 13)
            toks.append("-" + digits(k, True) + "." + digits(14 - k, False))
        assert all(len(t) <= 16 for t in toks) and all(len(t) == 16 for t in toks[-1024:])
        rows = [("[" + ", ".join(toks[i:i + 256]) + "]").encode() for i in range(0, len(toks), 256)]
        _CACHE["edge"] = rows
    return _CACHE["edge"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn])
def test_rounding_and_dtype_edges(dtype):
    check_rows(_edge_tokens(), dtype, pad=-1.0)


def test_window_and_token_table_edges():
    rows = []
    for tok in (b"7", b"-12345678.12345", b"1234567890.12345"):
        assert len(tok) in (1, 15, 16)
        for pos in range(2048 - 20, 2048 + 5):
            head = b"[3, "
            rows.append(head + b" " * (pos - len(head)) + tok + b" ,\t-2.5]")
            rows.append(head + b"\n" * (pos - len(head)) + tok + b",4]")
    for T in (2047, 2048, 2049, 2064, 4096, 4097):
        body = b"[" + b"12.5,-0.25, " * ((T - 30) // 12)
        rows.append(body + b" " * (T - len(body) - 6) + b"-3.75]")
        assert len(rows[-1]) == T
        body = b"[" + b"6," * ((T - 20) // 2)  # 1024 tokens in a window
        rows.append(body + b" " * (T - len(body) - 17) + b"1234567890.12345]")
        assert len(rows[-1]) == T
    rows.append(b"[" + b"1," * 4999 + b"1]")      # 1024 tokens per window: starts[] full, four trips a thread
    rows.append(b" [" + b"1," * 4999 + b"1]")     # the same, a token start on the window's last byte
    rows.append(b"[" + b"-1,9," * 2499 + b"-1,9]")
    rows.append(b"[ " + b"-1,9," * 2499 + b"-1,9 ]")
    rows.append(b"[1.5," + b" " * 5000 + b"-2]")
    rows.append(b"[" + b" \n\t\r" * 1250 + b"1.5," + b" " * 5000 + b"-2" + b" " * 3000 + b"]")
    check_rows(rows, torch.float32, L=5000, pad=-1.0)


# ----------------------------------------------------------------------------- F: device counting
def _corpus():
    """The count corpus, classified by the oracle, in batches with at most one row that must be
    flagged each (an err word holds one row index)."""
    if "corpus" not in _CACHE:
        rows = jo.count_corpus()
        info = [(t, jo.numbers(t), jo.simple_count(t), jo.guess(t)) for t in rows]
        flag = [r for r in info if r[1] is None and r[2] >= 0]
        rest = [r for r in info if not (r[1] is None and r[2] >= 0)]
        assert len(flag) > 1000 and sum(r[1] is not None and r[2] >= 0 for r in rest) > 80
        assert sum(r[1] is not None and r[2] < 0 for r in rest) > 50 and sum(r[1] is None for r in rest) > 40
        batches = []
        for i, f in enumerate(flag):
            b = rest[i::len(flag)]
            b.insert(i % (len(b) + 1), f)
            batches.append(b)
        _CACHE["corpus"] = batches
    return _CACHE["corpus"]


def _check_batch(res, b, rows, dtype, L, mode, mult, trunc, pad, what):
    """The user-level contract of one batch (rows: (text, numbers, simple_count, guess))."""
    fused = mode == "fused"
    n = len(rows)
    tr = trunc if trunc >= 0 else None
    keep = [min(c, trunc) if trunc >= 0 else c for c in (sc if sc >= 0 else g for _t, _v, sc, g in rows)]
    if fused:
        w = L
    else:
        w = max(keep)
        if mult > 1:
            w = _up(w, mult)
        w = min(w, L)
    r0 = int(res["row0"][b])
    host_rows = any(sc < 0 for _t, _v, sc, _g in rows)
    assert res["info"][b].tolist() == [w, int(host_rows), 1], (what, b, res["info"][b].tolist(), w, host_rows)
    out = res["out"][r0 * L:r0 * L + n * w].view(n, w)
    mask = res["mask"][r0 * L:r0 * L + n * w].view(n, w)
    lengths = res["lengths"][r0:r0 + n]
    desc = res["desc"][r0:r0 + n]
    err = int(res["err"][b])
    device = [v if v is not None and sc >= 0 else [] for _t, v, sc, _g in rows]
    exp, elen, emask = jo.expected(device, dtype, w, pad, tr)
    flagged = -1
    for i, (t, v, sc, g) in enumerate(rows):
        where = (what, b, i, t[:48], len(t))
        if v is not None and sc >= 0:
            assert int(lengths[i]) == int(elen[i]) == min(keep[i], w), where
            assert torch.equal(mask[i], emask[i].to(torch.uint8)), where
            continue
        if v is None and sc >= 0 and err == (ERR_TAG | i):
            flagged = i
            continue
        # left to the host: the guessed length, padding only, and the batch says so
        assert v is not None or sc < 0, (where, "neither flagged nor left to the host", err)
        assert int(lengths[i]) == min(g if tr is None else min(g, tr), w), where
        assert res["info"][b][1] == 1, where
        if not fused:
            assert desc[i].tolist()[1:] == [-2, g, min(g, trunc) if trunc >= 0 else g], (where, desc[i].tolist())
    assert err == (-1 if flagged < 0 else ERR_TAG | flagged), (what, b, err, flagged)
    sel = [i for i in range(n) if i != flagged]
    assert_same(out[sel], exp[sel], f"{what} batch {b}")
    if not fused and host_rows:
        assert int(res["ctr"][b, 1]) == (CTR_TAG << 32) | 1, (what, b)
    if not fused:
        assert int(res["ctr"][b, 0]) == (CTR_TAG << 32) | max(keep), (what, b)


RUNS = [("count", 8, 702), ("count", 1, 1000), ("fused", 0, 40)]


@pytest.mark.parametrize("trunc", [-1, 2])
@pytest.mark.parametrize("mode,mult,L", RUNS)
def test_count_corpus(mode, mult, L, trunc):
    batches = _corpus()
    res = run_group([[r[0] for r in b] for b in batches], torch.float32, L, mode, mult=mult, trunc=trunc, pad=-1.0)
    for b, rows in enumerate(batches):
        _check_batch(res, b, rows, torch.float32, L, mode, mult, trunc, -1.0, f"{mode} mult={mult} trunc={trunc}")


def test_count_corpus_bf16():
    batches = _corpus()
    res = run_group([[r[0] for r in b] for b in batches], torch.bfloat16, 702, "count", mult=8, pad=0.5)
    for b, rows in enumerate(batches):
        _check_batch(res, b, rows, torch.bfloat16, 702, "count", 8, -1, 0.5, "count bf16")


@pytest.mark.parametrize("mode,mult", [("count", 1), ("fused", 0)])
def test_descriptor_beyond_vals_cap_is_flagged(mode, mult):
    """Row 2's text ends beyond the batch's ``vals_cap``.  The buffer really holds valid text there,
    so a broken guard parses in-bounds memory and fails the assertions instead of faulting."""
    rows = [b"[1, 2]", b"[3]", b"[4, 5, 6, 7]"]
    # staged at 0, 16 and 32 (48 bytes): a cap of 40 ends inside row 2's 16-byte piece
    res = run_group([rows, [b"[8]"]], torch.float32, 4, mode, mult=mult, pad=-1.0, cap_cut={0: 40})
    assert res["err"].tolist() == [ERR_TAG | 2, -1]
    out = res["out"]
    w = 4 if mode == "fused" else 2  # the rows that were counted: 2 and 1 elements
    assert res["info"].tolist() == [[w, 0, 1], [4 if mode == "fused" else 1, 0, 1]]
    o = out[:3 * w].view(3, w)
    assert o[0, :2].tolist() == [1.0, 2.0] and o[1, :2].tolist() == [3.0, -1.0]
    assert o[2].tolist() == [-1.0] * w  # never parsed as values
    assert res["lengths"][:3].tolist() == [2, 1, 0]
    assert out[3 * 4:3 * 4 + 1].tolist() == [8.0] and int(res["lengths"][3]) == 1
