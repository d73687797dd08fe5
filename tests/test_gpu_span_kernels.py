"""span_decode_kernel and varlen_span_kernel at the kernel level (``launch_span_group`` /
``launch_var_span_group``: a launch filled from Python, plain device memory), against an oracle
that makes no call into the package (tests/helpers/span_oracle.py: a table CRC32C built from the
polynomial, a byte-string "log"; tests/helpers/known_records.py: plain-torch expected values).

Every launch writes into canary-filled outputs with guard rows on both sides, ``err`` preset to
-1 and ``partials`` preset to a sentinel, each with guard words: whatever the kernel has no
business writing must still hold its preset value.  Comparisons are exact.

* CRC value sweep: the raw partial CRC of segments without rows, at the window-geometry edges
  and every source alignment, alone and split over 2, 4 and 8 workgroups (twice back to back on one
  set of accumulator words, which must read zero afterwards);
* verdicts of whole segments, the chain of a RecordBatch cut into segments;
* fixed-width values: rows straddling a window boundary at every offset of a 16-byte group, rows
  cut by the segment's edges, every row-width path (G = 31, 32, 128, 129), every source size;
* var-len rows, host-row pseudo-segments, row tables that disagree with their segment.

tests/test_span_oracle.py proves the oracle and the inputs on the CPU, and holds the checks of
what the launch functions reject.
"""
import random
from collections import namedtuple

import numpy as np
import pytest
import torch

from helpers import span_oracle as so
from helpers.known_records import (assert_same, bits, esize, expected_fixed, expected_varlen, known_rows, known_values,
                                   norm_vectors, row_bytes)

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float8_e4m3fn: 3, torch.uint8: 4, torch.int8: 5,
      torch.int32: 6, torch.int64: 7}
GUARD = 2              # guard rows before and after every output
CANARY = 0xA5          # every byte of an untouched output (no NaN in any float type)
CANARY32 = -1515870811  # 0xA5A5A5A5 as int32
SENT = 0x5EA15EA1      # an untouched partial CRC word
NP = 48                # partial words per batch (segment indices 0..47)
f32, f16, bf16, fp8 = torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn
u8, i8, i32, i64 = torch.uint8, torch.int8, torch.int32, torch.int64

Seg = namedtuple("Seg", "pos len flags crc rb re batch seg", defaults=(0, 0, 0, 0, 0))
_CACHE = {}


def H():
    from torchkafka_amd.ops.native import hip

    return hip()


def core():
    from torchkafka_amd.ops.native import core as c

    return c()


def win():
    W = H().SPAN_WIN
    assert W == 10240 and H().SPAN_PIECE == 20 and H().MAX_LAUNCH_SEGS == NP
    return W


def crc_flags(first, last):
    h = H()
    return h.SEG_CRC | (h.SEG_CRC_FIRST if first else 0) | (h.SEG_CRC_LAST if last else 0)


def tabs():
    if "tabs" not in _CACHE:
        t = np.array(core().span_tables(), dtype=np.uint32)
        assert t.size == H().SPAN_TAB_WORDS
        _CACHE["tabs"] = torch.from_numpy(t.view(np.int32).copy()).cuda()
    return _CACHE["tabs"]


def stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------- preset words and outputs
class Status:
    """``err`` and ``partials`` of a launch's batches, preset, with guard words around each."""

    def __init__(self, nb):
        self.nb = nb
        self.err = torch.full((nb + 2,), -1, dtype=torch.int32, device="cuda")
        self.part = torch.full((nb + 2, NP + 2), SENT, dtype=torch.int32, device="cuda")

    def err_ptrs(self):
        return [self.err.data_ptr() + 4 * (k + 1) for k in range(self.nb)]

    def part_ptrs(self):
        return [self.part.data_ptr() + 4 * ((k + 1) * (NP + 2) + 1) for k in range(self.nb)]

    def check(self, err=None, partials=None, what=""):
        """``err``: {batch: segment}; ``partials``: {(batch, seg): raw CRC}.  Every other word must
        hold its preset value."""
        e = self.err.cpu().numpy()
        p = self.part.cpu().numpy().view(np.uint32)
        for k in range(-1, self.nb + 1):
            want = (err or {}).get(k, -1)
            assert int(e[k + 1]) == want, (what, "err of batch", k, int(e[k + 1]), want)
        wp = np.full((self.nb + 2, NP + 2), SENT, dtype=np.uint32)
        for (k, s), v in (partials or {}).items():
            wp[k + 1, s + 1] = v
        bad = np.argwhere(p != wp)
        assert bad.size == 0, (what, "partials (batch, seg, got, want)",
                               [(int(k) - 1, int(s) - 1, hex(int(p[k, s])), hex(int(wp[k, s]))) for k, s in bad[:8]])


class PartAcc:
    """The accumulator words of segment parts: zeroed once, guard pairs around them."""

    def __init__(self):
        self.t = torch.zeros((NP + 2, 2), dtype=torch.int32, device="cuda")
        self.t[0] = CANARY32
        self.t[-1] = CANARY32
        self.ptr = self.t.data_ptr() + 8

    def check_zero(self, what=""):
        a = self.t.cpu()
        assert bool((a[1:-1] == 0).all()), (what, "accumulator words left non-zero", a[1:-1].nonzero()[:8].tolist())
        assert bool((a[0] == CANARY32).all()) and bool((a[-1] == CANARY32).all()), (what, "accumulator guards")


def canary(rows, width, dt, device="cuda"):
    """[GUARD + rows + GUARD, width] of ``dt``, every byte CANARY."""
    n = (rows + 2 * GUARD) * width
    return torch.full((n * esize(dt),), CANARY, dtype=torch.uint8, device=device).view(dt).view(rows + 2 * GUARD, width)


def inner_ptr(t):
    return t.data_ptr() + GUARD * t.shape[1] * t.element_size()


def upload(lb):
    if not hasattr(lb, "_dev"):
        lb._dev = lb.upload()
    return lb._dev


def whole(lb, pos, n, rb=0, re=0, batch=0, seg=0):
    """A segment holding one whole RecordBatch as far as the kernel can tell: First|Last, the
    oracle's checksum of its bytes from byte 21."""
    return Seg(pos, n, crc_flags(True, True), so.crc32c(lb.bytes_at(pos, n)[so.FRONT:]), rb, re, batch, seg)


def launch_fixed(lb, segs, outs, row_pos, st, RE=4, src=f32, dst=f32, vec=False, parts=1, acc=None, shift=None,
                 scale=None, ext=None):
    _t, addr0 = upload(lb)
    ext = ext or [(0, 0, 0)] * st.nb
    H().launch_span_group(
        src=[addr0 + (s.pos - lb.base) for s in segs], log_pos=[s.pos for s in segs], len=[s.len for s in segs],
        flags=[s.flags for s in segs], crc=[s.crc for s in segs], row_begin=[s.rb for s in segs],
        row_end=[s.re for s in segs], batch=[s.batch for s in segs], seg=[s.seg for s in segs],
        out=outs, row_pos=row_pos, err=st.err_ptrs(), partials=st.part_ptrs(), ext_out=[e[0] for e in ext],
        ext_src=[e[1] for e in ext], ext_words=[e[2] for e in ext], row_elems=RE, vec_store=vec,
        tabs=tabs().data_ptr(), parts=parts, part_acc=acc.ptr if parts > 1 else 0, src_dtype=DT[src],
        dst_dtype=DT[dst], shift=shift.data_ptr() if shift is not None else 0,
        scale=scale.data_ptr() if scale is not None else 0, stream=stream())


def no_rows():
    """An output and a row table for launches whose segments carry no rows."""
    out = canary(1, 4, f32)
    rp = torch.zeros(1, dtype=torch.int64, device="cuda")
    return out, rp


def untouched(t, what=""):
    assert bool((t.cpu().view(-1).view(torch.uint8) == CANARY).all()), (what, "a canary-only output was written")


# ----------------------------------------------------------------------------- CRC value sweep
def _sweep():
    if "sweep" not in _CACHE:
        W = win()
        lb = so.LogBuilder(11)
        items = []
        for a in range(16):
            for n, first, last in so.sweep_cases(W, core().SPAN_SEG_MAX):
                items.append((lb.place(so.sweep_data(n), a), n, first, last))
        upload(lb)
        _CACHE["sweep"] = (lb, items)
    return _CACHE["sweep"]


def _run_sweep(parts, acc, out, rp):
    lb, items = _sweep()
    runs = []
    for i0 in range(0, len(items), NP):
        chunk = items[i0:i0 + NP]
        st = Status(3)
        segs = [Seg(pos, n, crc_flags(first, last), 0x01234567 + i, 0, 0, i % 3, i)
                for i, (pos, n, first, last) in enumerate(chunk)]
        launch_fixed(lb, segs, [inner_ptr(out)] * 3, [rp.data_ptr()] * 3, st, parts=parts, acc=acc)
        want = {(i % 3, i): so.sweep_raw(n, first) for i, (_pos, n, first, _last) in enumerate(chunk)}
        runs.append((st, want, [(n, first, last, (pos - lb.base) & 15) for pos, n, first, last in chunk]))
    return runs


@pytest.mark.parametrize("parts", [1, 2, 4, 8])
def test_crc_value_sweep(parts):
    """``partials[seg]`` of segments without rows equals the oracle's raw CRC: middle, last and first
    pieces of 1 byte to kSpanSegMax, at every ``src & 15``, 48 segments a launch.  With parts the
    sweep runs twice on one set of accumulator words that nothing zeroes in between."""
    acc = PartAcc()
    out, rp = no_rows()
    runs = []
    for _ in range(2 if parts > 1 else 1):
        runs += _run_sweep(parts, acc, out, rp)
    torch.cuda.synchronize()
    for j, (st, want, cases) in enumerate(runs):
        st.check(partials=want, what=f"parts {parts}, launch {j}: (len, first, last, src & 15) by seg = {cases}")
    acc.check_zero(f"parts {parts}")
    untouched(out)


# ----------------------------------------------------------------------------- verdicts
def _verdict_log():
    if "verdict" not in _CACHE:
        W = win()
        lb = so.LogBuilder(12)
        good, bad = [], []
        k = 0
        for n in (61, 81, W, W + 1, 2 * W + 21, 3 * W + 7):
            data = so.sweep_data(n, 5)
            crc = so.crc32c(data[so.FRONT:])

            def add(d, c, is_bad, why):
                nonlocal k
                (bad if is_bad else good).append((lb.place(d, (5 * k) % 16), n, c, why))
                k += 1

            add(data, crc, False, "clean")
            add(data, crc ^ (1 << (n % 32)), True, "crc bit")
            flips = {20, so.FRONT, n - 1}
            for w in range(1, -(-n // W)):
                flips |= {n - w * W - 1, n - w * W}  # the windows end at the segment's end
            for f in sorted(x for x in flips if 0 <= x < n):
                d = bytearray(data)
                d[f] ^= 0x10
                add(d, crc, f >= so.FRONT, f"byte {f} of {n}")  # bytes below 21 are outside the CRC
        upload(lb)
        _CACHE["verdict"] = (lb, good, bad)
    return _CACHE["verdict"]


def _run_verdicts(parts, acc, out, rp):
    lb, good, bad = _verdict_log()
    WHOLE = crc_flags(True, True)
    gi = 0
    runs = []

    def clean(batch, seg):
        nonlocal gi
        pos, n, c, _why = good[gi % len(good)]
        gi += 1
        return Seg(pos, n, WHOLE, c, 0, 0, batch, seg)

    nb = H().MAX_GROUP
    for i0 in range(0, len(bad), nb - 1):  # one bad segment per batch; the last batch stays clean
        segs, want, why = [], {}, {}
        for k, (pos, n, c, w) in enumerate(bad[i0:i0 + nb - 1]):
            s = 0
            for _ in range(k % 3):
                segs.append(clean(k, s))
                s += 1
            segs.append(Seg(pos, n, WHOLE, c, 0, 0, k, s))
            want[k], why[k] = s, w
            segs.append(clean(k, s + 1))
        segs += [clean(nb - 1, 0), clean(nb - 1, 1)]
        st = Status(nb)
        launch_fixed(lb, segs, [inner_ptr(out)] * nb, [rp.data_ptr()] * nb, st, parts=parts, acc=acc)
        runs.append((st, want, why))
    # several bad segments in one batch: the word keeps the lowest, whichever workgroup finishes
    # last (a 61-byte segment is done long before one of four windows)
    small = [b for b in bad if b[1] == 61]
    big = [b for b in bad if b[1] > 3 * win()]

    def broken(b, batch, seg):
        return Seg(b[0], b[1], WHOLE, b[2], 0, 0, batch, seg)

    segs = [clean(0, 0), broken(small[0], 0, 1), clean(0, 2), broken(big[0], 0, 3),
            clean(1, 0), broken(big[1], 1, 1), broken(small[1], 1, 2), broken(small[2], 1, 3),
            broken(big[2], 2, 0), broken(small[0], 2, 1), broken(big[3], 2, 2),
            clean(3, 0), clean(3, 1), broken(big[-1], 3, 2), broken(big[-2], 3, 3), broken(small[-1], 3, 4),
            clean(4, 0)]
    st = Status(5)
    launch_fixed(lb, segs, [inner_ptr(out)] * 5, [rp.data_ptr()] * 5, st, parts=parts, acc=acc)
    runs.append((st, {0: 1, 1: 1, 2: 0, 3: 2}, {0: "several bad segments in a batch"}))
    return runs


@pytest.mark.parametrize("parts", [1, 2, 4, 8])
def test_whole_segment_verdicts(parts):
    """Whole segments: the right checksum leaves ``err`` at -1; one wrong bit in ``crc`` or one
    flipped byte (the first CRC'd byte, the last, both sides of every window boundary) stores the
    segment's index in its own batch's word only; with several bad segments in a batch the word
    holds the lowest of them; a flipped byte 20 is not caught; nothing touches ``partials``."""
    acc = PartAcc()
    out, rp = no_rows()
    runs = []
    for _ in range(2 if parts > 1 else 1):
        runs += _run_verdicts(parts, acc, out, rp)
    torch.cuda.synchronize()
    for j, (st, want, why) in enumerate(runs):
        st.check(err=want, what=f"parts {parts}, launch {j}: {why}")
    acc.check_zero(f"parts {parts}")
    untouched(out)


@pytest.mark.parametrize("parts", [1, 8])
def test_partials_chain_to_the_record_batch_crc(parts):
    """A 300,000-byte RecordBatch cut at 131,072 and 150,001 (and once more: a segment holds at most
    kSpanSegMax bytes): the device partials, combined as batch_verdicts.cpp combines them, give the
    oracle's checksum of the run."""
    c = core()
    data = so.sweep_data(300_000, 4)
    cuts = [0, 131_072, 150_001, 150_001 + 131_072, 300_000]
    lb = so.LogBuilder(13)
    p0 = lb.place(data, 3)
    want_crc = so.crc32c(data[so.FRONT:])
    segs, want = [], {}
    for i in range(len(cuts) - 1):
        lo, hi = cuts[i], cuts[i + 1]
        segs.append(Seg(p0 + lo, hi - lo, crc_flags(i == 0, i == len(cuts) - 2), want_crc, 0, 0, 0, i + 2))
        want[(0, i + 2)] = so.segment_raw(data[lo:hi], i == 0)
    acc = PartAcc()
    out, rp = no_rows()
    st = Status(1)
    launch_fixed(lb, segs, [inner_ptr(out)], [rp.data_ptr()], st, parts=parts, acc=acc)
    torch.cuda.synchronize()
    st.check(partials=want, what="chain")
    p = st.part.cpu().numpy().view(np.uint32)
    got = 0
    for i, s in enumerate(segs):
        crc_len = s.len - (so.FRONT if i == 0 else 0)
        got = c.crc32c_shift_raw(got, crc_len) ^ int(p[1, s.seg + 1])
    assert got ^ 0xFFFFFFFF == want_crc
    acc.check_zero()
    untouched(out)


# ----------------------------------------------------------------------------- fixed-width values
def fill_rows(lb, rb, until, rng):
    """Reserves rows of ``rb`` bytes behind 3-13 framing bytes each while they end before ``until``."""
    pos = []
    while True:
        gap = rng.randrange(3, 14)
        if lb.pos() + gap + rb > until:
            return pos
        lb.frame(gap)
        pos.append(lb.reserve(rb))


def write_rows(lb, pos, rows):
    raw = row_bytes(rows)
    rb = len(raw) // max(1, len(pos))
    for i, p in enumerate(pos):
        lb.write(p, raw[i * rb:(i + 1) * rb])


def vec_allowed(RE, src, dst):
    per = 16 // esize(src)
    return RE % per == 0 and (RE * esize(dst)) % 16 == 0


def norm_of(RE, norm):
    if not norm:
        return None, None, None, None
    mean, std = norm_vectors(RE, RE)
    return mean, std, mean.cuda(), (1.0 / std).cuda()


def run_fixed(lb, segs, pos, rows, expect, RE, src, dst, vec, parts=1, norm=False, err=None, partials=None, what=""):
    """One launch of one batch over ``rows`` at ``pos``; ``expect``: the whole output, guards included."""
    _mean, _std, shift, scale = norm_of(RE, norm)
    out = canary(len(pos), RE, dst)
    rp = torch.tensor(pos, dtype=torch.int64).cuda()
    st = Status(1)
    acc = PartAcc()
    launch_fixed(lb, segs, [inner_ptr(out)], [rp.data_ptr()], st, RE, src, dst, vec, parts, acc, shift, scale)
    torch.cuda.synchronize()
    assert_same(out.cpu(), expect, what)
    st.check(err=err, partials=partials, what=what)
    acc.check_zero(what)


def expect_rows(rows, RE, dst, norm=False):
    mean, std, _sh, _sc = norm_of(RE, norm)
    e = canary(rows.shape[0], RE, dst, "cpu")
    bits(e)[GUARD:GUARD + rows.shape[0]] = bits(expected_fixed(rows, dst, mean, std))
    return e


# (src, dst, row_elems, normalise): every source size, G = 31, 32, 128, 129 groups a row (the kernel
# spreads rows of < 32 groups as (row, group) pairs, gives longer ones a wave, ones of > 128 every
# wave), whole and short last groups
STRADDLE = [
    (f32, f32, 24, True), (f32, bf16, 24, False), (f32, bf16, 124, False), (f32, f32, 123, False),
    (f32, f32, 128, False), (f32, f16, 128, True), (f32, fp8, 512, False), (f32, f32, 516, False),
    (f32, bf16, 513, True), (u8, f32, 48, True), (u8, f32, 2049, False), (i8, bf16, 512, False),
    (f16, f32, 256, False), (bf16, f32, 250, False), (i32, i64, 128, False), (i32, f32, 20, False),
    (i64, i64, 64, False), (i64, i32, 7, False),
]


@pytest.mark.parametrize("src,dst,RE,norm", STRADDLE, ids=lambda v: str(v).replace("torch.", ""))
def test_fixed_rows_straddling_window_boundaries(src, dst, RE, norm):
    """16 segments of two windows (every fourth: four, the ring wraps), the window boundary falling
    o = 0..15 bytes into a 16-byte group of a row; every ``src & 15``; vector stores off and on."""
    W = win()
    rb = RE * esize(src)
    g = 1 if rb < 64 else 2
    assert 16 * g + 15 < rb
    rng = random.Random(RE)
    lb = so.LogBuilder(100 + RE)
    pos, bounds = [], []
    for o in range(16):
        S = lb.place(b"", (7 * o + 3) % 16)
        lb.frame(rng.randrange(1, 30))
        p = fill_rows(lb, rb, lb.pos() + 40 + 2 * rb, rng)
        lb.frame(rng.randrange(1, 14))
        p.append(lb.reserve(rb))
        hi = p[-1] + 16 * g + o + (3 * W if o % 4 == 3 else W)
        p += fill_rows(lb, rb, hi - 1, rng)
        lb.frame(hi - lb.pos())
        bounds.append((S, hi - S, len(pos), len(pos) + len(p)))
        pos += p
        assert len(p) <= core().SPAN_MAX_SEG_ROWS and hi - S <= core().SPAN_SEG_MAX
    rows = known_rows(src, (RE,), len(pos), RE)
    write_rows(lb, pos, rows)
    segs = [whole(lb, S, n, r0, r1, 0, i) for i, (S, n, r0, r1) in enumerate(bounds)]
    for vec in (False, True) if vec_allowed(RE, src, dst) else (False,):
        for nm in (False, True) if norm else (False,):
            run_fixed(lb, segs, pos, rows, expect_rows(rows, RE, dst, nm), RE, src, dst, vec, norm=nm,
                      what=f"vec {vec} norm {nm}")


@pytest.mark.parametrize("src,dst,RE", [(f32, f32, 5000), (f32, bf16, 40), (i64, i64, 33), (u8, f32, 100),
                                        (f32, f16, 516)], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("parts", [1, 4])
def test_fixed_rows_cut_by_segment_edges(src, dst, RE, parts):
    """Three rows; the run is cut inside the middle one, in the middle of a 16-byte group and at the
    start of one.  Each half alone writes only its own elements (the rest stays canary), both halves
    in one launch deliver the row; the raw CRCs of the two pieces land in ``partials``."""
    es = esize(src)
    per = 16 // es
    rb = RE * es
    for cut_el in ((RE // 2) // per * per + 1 if per > 1 else RE // 2, (RE // 3) // per * per):
        rng = random.Random(RE + cut_el)
        lb = so.LogBuilder(200 + RE + cut_el)
        S = lb.place(b"", (RE + cut_el) % 16)
        lb.frame(9)
        pos = fill_rows(lb, rb, lb.pos() + 3 * (rb + 14), rng)[:3]
        assert len(pos) == 3
        lb.frame(5)
        end = lb.pos()
        rows = known_rows(src, (RE,), 3, RE + cut_el)
        write_rows(lb, pos, rows)
        cut = pos[1] + cut_el * es
        A = Seg(S, cut - S, crc_flags(True, False), 0, 0, 2, 0, 0)
        B = Seg(cut, end - cut, crc_flags(False, True), 0, 1, 3, 0, 1)
        pa = {(0, 0): so.segment_raw(lb.bytes_at(S, cut - S), True)}
        pb = {(0, 1): so.segment_raw(lb.bytes_at(cut, end - cut), False)}
        full = expect_rows(rows, RE, dst)
        ea, eb = full.clone(), full.clone()
        can = canary(3, RE, dst, "cpu")
        ea[GUARD + 1, cut_el:] = can[GUARD + 1, cut_el:]
        ea[GUARD + 2] = can[GUARD + 2]
        eb[GUARD] = can[GUARD]
        eb[GUARD + 1, :cut_el] = can[GUARD + 1, :cut_el]
        for vec in (False, True) if vec_allowed(RE, src, dst) else (False,):
            run_fixed(lb, [A], pos, rows, ea, RE, src, dst, vec, parts, partials=pa, what=f"first half, cut {cut_el}")
            run_fixed(lb, [B], pos, rows, eb, RE, src, dst, vec, parts, partials=pb, what=f"second half, cut {cut_el}")
            run_fixed(lb, [A, B], pos, rows, full, RE, src, dst, vec, parts, partials={**pa, **pb},
                      what=f"both halves, cut {cut_el}")


@pytest.mark.parametrize("parts", [1, 2])
def test_fixed_2048_rows_in_one_segment(parts):
    """kSpanMaxSegRows rows of 3 int32 (one short group each) in one segment of four windows."""
    n = core().SPAN_MAX_SEG_ROWS
    rng = random.Random(2048)
    lb = so.LogBuilder(2048)
    S = lb.place(b"", 13)
    pos = []
    for _ in range(n):
        lb.frame(rng.randrange(1, 10))
        pos.append(lb.reserve(12))
    lb.frame(3)
    rows = known_rows(i32, (3,), n, 2048)
    write_rows(lb, pos, rows)
    seg = whole(lb, S, lb.pos() - S, 0, n, 0, 5)
    assert seg.len > 3 * win()
    for dst in (i64, f32):
        run_fixed(lb, [seg], pos, rows, expect_rows(rows, 3, dst), 3, i32, dst, False, parts, what=str(dst))


@pytest.mark.parametrize("RE", [24, 128, 516])
def test_fixed_listed_rows_outside_the_segment_are_left_alone(RE):
    """Rows in ``[row_begin, row_end)`` that do not intersect the segment (they lie before and after
    it in the log) are not written."""
    rb = RE * 4
    rng = random.Random(RE)
    lb = so.LogBuilder(300 + RE)
    lb.align(5, so.SLACK)
    before = fill_rows(lb, rb, lb.pos() + 2 * (rb + 14), rng)
    lb.frame(1)
    S = lb.pos()
    lb.frame(4)
    inside = fill_rows(lb, rb, lb.pos() + win() + 3 * (rb + 14), rng)
    lb.frame(2)
    end = lb.pos()
    after = fill_rows(lb, rb, lb.pos() + 2 * (rb + 14), rng)
    pos = before + inside + after
    assert len(before) == 2 and len(after) == 2 and end - S > win()
    rows = known_rows(f32, (RE,), len(pos), RE)
    write_rows(lb, pos, rows)
    e = expect_rows(rows, RE, bf16)
    can = canary(len(pos), RE, bf16, "cpu")
    for r in (0, 1, len(pos) - 2, len(pos) - 1):
        e[GUARD + r] = can[GUARD + r]
    run_fixed(lb, [whole(lb, S, end - S, 0, len(pos), 0, 0)], pos, rows, e, RE, f32, bf16, vec_allowed(RE, f32, bf16))


@pytest.mark.parametrize("parts", [1, 2])
def test_fixed_record_fields_copied_by_segment_zero_only(parts):
    """``ext_words`` int64 words go from ``ext_src`` to ``ext_out`` in the workgroup of the batch's
    segment 0: a launch holding only later segments of a batch leaves its ``ext_out`` alone."""
    RE, rb = 8, 32
    rng = random.Random(8)
    lb = so.LogBuilder(8)
    bounds, pos = [], []
    for i in range(4):
        S = lb.place(b"", 3 * i)
        lb.frame(6)
        p = fill_rows(lb, rb, lb.pos() + 600, rng)
        lb.frame(4)
        bounds.append((S, lb.pos() - S, len(p)))
        pos.append(p)
    rows = [known_rows(f32, (RE,), len(p), 80 + i) for i, p in enumerate(pos)]
    for p, r in zip(pos, rows):
        write_rows(lb, p, r)
    # batch 0: segments 0 and 1; batch 1: segments 1 and 2 of some slot whose segment 0 went elsewhere
    n0, n1 = bounds[0][2] + bounds[1][2], bounds[2][2] + bounds[3][2]
    segs = [whole(lb, bounds[0][0], bounds[0][1], 0, bounds[0][2], 0, 0),
            whole(lb, bounds[1][0], bounds[1][1], bounds[0][2], n0, 0, 1),
            whole(lb, bounds[2][0], bounds[2][1], 0, bounds[2][2], 1, 1),
            whole(lb, bounds[3][0], bounds[3][1], bounds[2][2], n1, 1, 2)]
    outs = [canary(n0, RE, f32), canary(n1, RE, f32)]
    rps = [torch.tensor(pos[2 * k] + pos[2 * k + 1], dtype=torch.int64).cuda() for k in range(2)]
    words = [2 * n0 - 1, 2 * n1]
    esrc = [known_values(i64, w + 4, 90 + k).cuda() for k, w in enumerate(words)]
    eout = [canary(1, w + 4, i64) for w in words]  # 4 words past ext_words, then the guard rows
    st = Status(2)
    acc = PartAcc()
    launch_fixed(lb, segs, [inner_ptr(o) for o in outs], [r.data_ptr() for r in rps], st, RE, f32, f32, True, parts,
                 acc,
                 ext=[(inner_ptr(eout[k]), esrc[k].data_ptr(), words[k]) for k in range(2)])
    torch.cuda.synchronize()
    assert_same(outs[0].cpu(), expect_rows(torch.cat(rows[:2]), RE, f32), "batch 0")
    assert_same(outs[1].cpu(), expect_rows(torch.cat(rows[2:]), RE, f32), "batch 1")
    want0 = canary(1, words[0] + 4, i64, "cpu")
    want0[GUARD, :words[0]] = esrc[0].cpu()[:words[0]]
    assert torch.equal(eout[0].cpu(), want0)
    untouched(eout[1], "ext_out of a batch without its segment 0")
    st.check()
    acc.check_zero()


# ----------------------------------------------------------------------------- var-len rows
ROW_DT = np.dtype([("pos", "<u8"), ("tlen", "<i4"), ("count", "<i4")])
assert ROW_DT.itemsize == 16


def launch_var(lb, segs, b, st, src, dst, pad, parts=1, acc=None):
    """``b``: per batch a dict(out, rows, slot, lengths, mask, L, trunc, aligned) of addresses / values."""
    _t, addr0 = upload(lb)
    host = H().SEG_HOST_ROWS
    H().launch_var_span_group(
        src=[0 if s.flags & host else addr0 + (s.pos - lb.base) for s in segs], log_pos=[s.pos for s in segs],
        len=[s.len for s in segs], flags=[s.flags for s in segs], crc=[s.crc for s in segs],
        row_begin=[s.rb for s in segs], row_end=[s.re for s in segs], batch=[s.batch for s in segs],
        seg=[s.seg for s in segs], out=[x["out"] for x in b], rows=[x["rows"] for x in b],
        slot=[x["slot"] for x in b], lengths=[x["lengths"] for x in b], mask=[x["mask"] for x in b],
        err=st.err_ptrs(), partials=st.part_ptrs(), L=[x["L"] for x in b], trunc_len=[x["trunc"] for x in b],
        aligned=[x["aligned"] for x in b], tabs=tabs().data_ptr(), parts=parts,
        part_acc=acc.ptr if parts > 1 else 0, src_dtype=DT[src], dst_dtype=DT[dst], pad=pad, stream=stream())


def var_aligned_allowed(src, dst, L):
    g = 16 // esize(src) * esize(dst)
    return g >= 16 and g % 16 == 0 and (L * esize(dst)) % 16 == 0


class VarBatch:
    """Rows of one var-len batch: ``table`` holds (pos, tlen, count) as the kernel is told them,
    ``values`` the elements each row must deliver (a tensor of the source dtype)."""

    def __init__(self):
        self.table, self.values = [], []

    def add(self, pos, tlen, count, values):
        self.table.append((pos, tlen, count))
        self.values.append(values)
        return len(self.table) - 1

    def run_args(self, dst, L, trunc, aligned, with_ml, slot):
        n = len(self.table)
        self.out = canary(n, L, dst)
        self.lengths = canary(n, 1, i64) if with_ml else None
        self.mask = canary(n, L, u8) if with_ml else None
        self.rows_dev = torch.from_numpy(np.array(self.table, dtype=ROW_DT).view(np.uint8).copy()).cuda()
        return {"out": inner_ptr(self.out), "rows": self.rows_dev.data_ptr(), "slot": slot,
                "lengths": inner_ptr(self.lengths) if with_ml else 0, "mask": inner_ptr(self.mask) if with_ml else 0,
                "L": L, "trunc": trunc, "aligned": aligned}

    def check(self, dst, L, pad, trunc, with_ml, what, values=None):
        n = len(self.table)
        out, lengths, mask = expected_varlen(values or self.values, dst, L, pad, None if trunc < 0 else trunc)
        e = canary(n, L, dst, "cpu")
        e[GUARD:GUARD + n] = out
        assert_same(self.out.cpu(), e, what)
        if with_ml:
            el = canary(n, 1, i64, "cpu")
            el[GUARD:GUARD + n, 0] = lengths
            assert torch.equal(self.lengths.cpu(), el), (what, "lengths")
            em = canary(n, L, u8, "cpu")
            em[GUARD:GUARD + n] = mask.to(u8)
            assert torch.equal(self.mask.cpu(), em), (what, "mask")


def _var_case(src, L):
    """16 segments of two windows over rows of 0, 1, kPer - 1, kPer, kPer + 1 and more elements
    behind 1-9 framing bytes (every byte alignment), the window boundary falling o = 0..15 bytes
    into a 16-byte unit of a row; two batches; rows the worker copied (tlen -1) in a slot buffer
    with their kSegHostRows pseudo-segments.  -> (log, segments, batches, slot tensor)."""
    key = ("var", src, L)
    if key in _CACHE:
        return _CACHE[key]
    W = win()
    es = esize(src)
    per = 16 // es
    counts = [0, 1, per - 1, per, per + 1, 40, L + 52, 17, 3 * per, L, L + 1, 2]
    rng = random.Random(per)
    lb = so.LogBuilder(400 + es)
    batches = [VarBatch(), VarBatch()]
    slot = bytearray()
    bounds = []
    seed = [0]

    def vals(n):
        seed[0] += 1
        return known_values(src, n, 7000 + seed[0])

    def host_row(vb, n):
        at = len(slot)
        v = vals(n)
        slot.extend(row_bytes(v))
        slot.extend(bytes((-len(slot)) & 15))
        return vb.add(at, -1, n, v)

    def log_row(vb, n):
        lb.frame(rng.randrange(1, 10))
        v = vals(n)
        return vb.add(lb.put(row_bytes(v)), n * es, n, v)

    for o in range(16):
        vb = batches[o // 8]
        S = lb.place(b"", (11 * o + 1) % 16)
        r0 = len(vb.table)
        for j in range(6):
            log_row(vb, counts[(o + j) % len(counts)])
        if o % 8 == 2:
            mid = host_row(vb, 23)  # a worker-copied row inside a log segment's row range
            bounds.append((None, 0, mid, mid + 1, o // 8))
        r = log_row(vb, 40)
        hi = vb.table[r][0] + 16 + o + W
        j = 0
        while lb.pos() + 10 + es * (L + 52) < hi:
            log_row(vb, counts[j % len(counts)])
            j += 1
        lb.frame(hi - lb.pos())
        assert len(vb.table) - r0 <= core().JSON_SPAN_MAX_SEG_ROWS
        bounds.append((S, hi - S, r0, len(vb.table), o // 8))
    for k, vb in enumerate(batches):
        r0 = len(vb.table)
        for n in (100, 0, per + 1, L):
            host_row(vb, n)
        bounds.append((None, 0, r0, len(vb.table), k))
    host = H().SEG_HOST_ROWS
    segs, nseg = [], [0, 0]
    for S, n, r0, r1, k in bounds:
        if S is None:
            segs.append(Seg(0, 0, host, 0, r0, r1, k, nseg[k]))
        else:
            segs.append(whole(lb, S, n, r0, r1, k, nseg[k]))
        nseg[k] += 1
    upload(lb)
    slot_t = torch.frombuffer(bytearray(slot) + bytes(64), dtype=torch.uint8).cuda()
    _CACHE[key] = (lb, segs, batches, slot_t)
    return _CACHE[key]


VAR_VARIANTS = [  # (aligned path, trunc_len, lengths and mask present, parts)
    (False, -1, True, 1), (True, -1, True, 1), (True, 30, False, 1), (False, 30, True, 4), (True, -1, True, 8),
    (False, -1, False, 2),
]


@pytest.mark.parametrize("src,dst", [(i32, i64), (i32, i32), (f32, bf16), (u8, i64), (i64, i64), (f16, f32),
                                     (i8, f32)], ids=lambda v: str(v).replace("torch.", ""))
def test_varlen_rows(src, dst):
    """Padded values, lengths and mask of var-len rows against ``expected_varlen``: rows of 0 to
    more than ``L`` elements at every byte alignment and across window boundaries, truncation,
    null ``lengths`` / ``mask``, the aligned vector-store path where the driver would take it,
    worker-copied rows, parts.  With parts above 1 the values are checked, not who wrote them: every
    part would write the same padding, mask and length, so a part other than 0 writing them too
    (duplicate stores) is not something this comparison can see."""
    L = 48
    lb, segs, batches, slot = _var_case(src, L)
    pad = 7 if not dst.is_floating_point else -1.5
    seen = set()
    for aligned, trunc, with_ml, parts in VAR_VARIANTS:
        aligned = aligned and var_aligned_allowed(src, dst, L)
        if (aligned, trunc, with_ml, parts) in seen:
            continue
        seen.add((aligned, trunc, with_ml, parts))
        what = f"aligned {aligned} trunc {trunc} lengths/mask {with_ml} parts {parts}"
        st = Status(2)
        acc = PartAcc()
        args = [vb.run_args(dst, L, trunc, aligned, with_ml, slot.data_ptr()) for vb in batches]
        for _ in range(2 if parts > 1 else 1):  # back to back on the same accumulator words
            launch_var(lb, segs, args, st, src, dst, pad, parts, acc)
        torch.cuda.synchronize()
        for k, vb in enumerate(batches):
            vb.check(dst, L, pad, trunc, with_ml, f"batch {k}, {what}")
        st.check(what=what)
        acc.check_zero(what)


@pytest.mark.parametrize("parts", [1, 2])
def test_varlen_row_table_that_disagrees_with_its_segment(parts):
    """A row whose ``count * sizeof(S)`` is not ``tlen``, one reaching past the segment's end and one
    starting before its first byte: ``err`` names the segment, the row is delivered as padding with
    length 0, every other row is right.  Two such segments in one batch: ``err`` names the lower."""
    L, es = 16, 4
    rng = random.Random(5)
    lb = so.LogBuilder(500)
    batches, bounds = [], []
    for kind in range(5):
        vb = VarBatch()
        want = []
        S0 = lb.place(b"", 2 + kind)  # a clean segment 0 of the batch
        for n in (3, 9):
            lb.frame(rng.randrange(1, 10))
            v = known_values(i32, n, 600 + n)
            vb.add(lb.put(row_bytes(v)), n * es, n, v)
            want.append(v)
        lb.frame(3)
        E0 = lb.pos()
        lb.align(7 * kind % 16, so.SLACK)
        S1 = lb.pos()
        lb.frame(3)
        rowpos = []
        for n in (5, 12, 7):
            lb.frame(rng.randrange(1, 10))
            v = known_values(i32, n, 610 + n + kind)
            rowpos.append(lb.put(row_bytes(v)))
            vb.add(rowpos[-1], n * es, n, v)
            want.append(v)
        lb.frame(6)
        E1 = lb.pos()
        empty = torch.zeros(0, dtype=i32)
        if kind == 0:    # the middle row's byte length disagrees with its count
            vb.table[3] = (rowpos[1], 12 * es + 1, 12)
            want[3] = empty
        elif kind == 1:  # the last row reaches past the segment's end
            E1 = rowpos[2] + 2 * es
            want[4] = empty
        elif kind == 2:  # the first row starts before the segment's first byte
            S1 = rowpos[0] + es
            want[2] = empty
        elif kind == 4:  # both segments of the batch hold a row whose length disagrees
            vb.table[1] = (vb.table[1][0], 9 * es - 1, 9)
            vb.table[3] = (rowpos[1], 12 * es + 1, 12)
            want[1] = want[3] = empty
        bounds.append((S0, E0, S1, E1))
        batches.append((vb, want))
    segs = []
    for k, (S0, E0, S1, E1) in enumerate(bounds):
        segs.append(whole(lb, S0, E0 - S0, 0, 2, k, 0))
        segs.append(whole(lb, S1, E1 - S1, 2, 5, k, 1))
    st = Status(5)
    acc = PartAcc()
    args = [vb.run_args(i64, L, -1, True, True, 0) for vb, _w in batches]
    launch_var(lb, segs, args, st, i32, i64, -3, parts, acc)
    torch.cuda.synchronize()
    for k, (vb, want) in enumerate(batches):
        vb.check(i64, L, -3, -1, True, f"batch {k}", values=want)
    st.check(err={0: 1, 1: 1, 2: 1, 4: 0}, what="row tables")  # batch 3 is consistent: clean
    acc.check_zero()
