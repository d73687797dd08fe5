"""The gfx950 pack kernel (csrc/hip/pack.hip) and ``pack_padded`` against a Python loop over the
rows (tests/helpers/packed.py): both launch shapes (one launch up to PACK_FUSED_ROWS rows, scan +
pack above), every element size, cuts at the capacity, lengths out of range, and -- through the raw
binding -- canaries around every output."""
import random

import pytest
import torch

from helpers.known_records import bits, known_values
from helpers.packed import capacities, check_packed, expected_packed, pad_element

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# element size -> a dtype of that size (the kernel moves bits: one dtype per size; fp8 rides along)
BY_SIZE = {1: torch.uint8, 2: torch.bfloat16, 4: torch.float32, 8: torch.int64}
WIDTHS = (0, 1, 7, 8, 9, 2049)


def _fused_rows() -> int:
    from torchkafka_amd.ops import hip

    return int(hip().PACK_FUSED_ROWS)


def _row_counts():
    f = _fused_rows()
    return [0, 1, 2, 63, 64, 65, 257, f - 1, f, f + 1]


def _lengths(rows: int, W: int, seed: int):
    """Random lengths holding 0 and W; the last row is full, so capacity total - 1 cuts inside it."""
    rng = random.Random(seed)
    lens = [rng.randint(0, W) for _ in range(rows)]
    if rows:
        lens[0], lens[-1] = 0, W
    if rows > 2:
        lens[rows // 2], lens[1] = W, 0
    return lens


def _padded(dt, rows: int, W: int, seed: int) -> torch.Tensor:
    src = torch.float32 if dt == torch.float8_e4m3fn else dt
    return known_values(src, rows * W, seed).to(dt).view(rows, W)


def _widths(rows: int):
    return [w for w in WIDTHS if w <= 9] if rows >= _fused_rows() - 1 else list(WIDTHS)


@pytest.mark.parametrize("k", range(10))
def test_pack_padded_matches_the_row_loop(k):
    from torchkafka_amd import pack_padded

    rows = _row_counts()[k]
    for W in _widths(rows):
        lens = _lengths(rows, W, 31 * rows + W)
        lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
        for esz, dt in BY_SIZE.items():
            padded = _padded(dt, rows, W, rows + W + esz)
            dev = padded.to(DEV)
            pad = -1 if esz != 4 else float("nan")
            for cap in capacities(lens, W):
                ids = (cap + esz) % 2 == 0
                pb = pack_padded(dev, lens_d, cap, pad, ids)
                assert pb.values.is_cuda and pb.values.numel() == cap
                check_packed(pb, padded, lens, cap, pad, ids, f"{rows}x{W} esz {esz} cap {cap}")
            pb = pack_padded(dev, lens_d)  # default capacity rows * W, pad 0
            check_packed(pb, padded, lens, rows * W, 0, False, f"{rows}x{W} esz {esz} default")


def test_pack_padded_fp8_and_int32_lengths():
    from torchkafka_amd import pack_padded

    rows, W = 65, 9
    lens = _lengths(rows, W, 5)
    padded = _padded(torch.float8_e4m3fn, rows, W, 9)
    pb = pack_padded(padded.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), None, -1, True)
    check_packed(pb, padded, lens, rows * W, -1, True, "fp8")


def test_pack_padded_takes_a_strided_view():
    from torchkafka_amd import pack_padded

    rows, W = 65, 7
    lens = _lengths(rows, W, 6)
    wide = _padded(torch.int64, rows, W + 3, 4)
    padded = wide[:, 1:W + 1]  # not contiguous
    pb = pack_padded(padded.to(DEV), torch.tensor(lens, device=DEV), None, -1, False)
    check_packed(pb, padded.contiguous(), lens, rows * W, -1, False, "strided")
    pb = pack_padded(wide.to(DEV)[:, 1:W + 1], torch.tensor(lens, device=DEV), None, -1, False)
    check_packed(pb, padded.contiguous(), lens, rows * W, -1, False, "strided on the device")


@pytest.mark.parametrize("rows", [5, 257, "fused+1"])
def test_lengths_out_of_range_are_clamped(rows):
    from torchkafka_amd import pack_padded

    rows = _fused_rows() + 1 if rows == "fused+1" else rows
    W = 9
    lens = _lengths(rows, W, 77)
    lens[0], lens[2], lens[-1] = -3, W + 4, W + 4
    padded = _padded(torch.int64, rows, W, 8)
    for cap in capacities(lens, W):
        pb = pack_padded(padded.to(DEV), torch.tensor(lens, device=DEV), cap, -1, True)
        check_packed(pb, padded, lens, cap, -1, True, f"clamped {rows} cap {cap}")


CANARY = 0xA5
GUARD = 512  # canary bytes before and after every output


def _canaried(n_elems: int, esz: int, off: int):
    """A canary-filled byte buffer holding an output of n_elems at element offset `off` behind the guard."""
    buf = torch.full((GUARD + (off + n_elems) * esz + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    return buf, GUARD + off * esz


def _intact(buf: torch.Tensor, start: int, nbytes: int) -> bool:
    b = buf.cpu()
    return bool((b[:start] == CANARY).all()) and bool((b[start + nbytes:] == CANARY).all())


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("rows,W,bad", [(65, 9, False), (65, 9, True), (3, 2049, False), ("fused+1", 7, True),
                                        (0, 9, False), (7, 0, False)])
def test_raw_binding_writes_nothing_outside_its_outputs(rows, W, bad, off):
    from torchkafka_amd.ops import hip

    rows = _fused_rows() + 1 if rows == "fused+1" else rows
    lens = _lengths(rows, W, rows + W)
    if bad and rows:
        lens[0], lens[-1] = W + 4, W + 4
        lens[1] = -3
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for esz, dt in BY_SIZE.items():
        padded = _padded(dt, rows, W, esz + rows)
        dev = padded.to(DEV)
        lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
        for cap in capacities(lens, W):
            vbuf, vo = _canaried(cap, esz, off)
            cbuf, co = _canaried(rows + 1, 4, off)
            tbuf, to = _canaried(1, 8, off)
            pbuf, po = _canaried(cap, 4, off)
            sbuf, so = _canaried(cap, 4, off)
            fill = int(bits(pad_element(dt, -1).reshape(1)).item()) & ((1 << (8 * esz)) - 1)
            hip().pack_rows(dev.data_ptr(), esz, rows, W, lens_d.data_ptr(), vbuf.data_ptr() + vo, cap, fill,
                            cbuf.data_ptr() + co, tbuf.data_ptr() + to, pbuf.data_ptr() + po, sbuf.data_ptr() + so,
                            stream)
            torch.cuda.synchronize()
            what = f"{rows}x{W} esz {esz} cap {cap} off {off}"
            for name, buf, o, nbytes in (("values", vbuf, vo, cap * esz), ("cu_seqlens", cbuf, co, (rows + 1) * 4),
                                         ("total", tbuf, to, 8), ("position_ids", pbuf, po, cap * 4),
                                         ("segment_ids", sbuf, so, cap * 4)):
                assert _intact(buf, o, nbytes), f"{what}: canary around {name} overwritten"
            values, cu, total, pos, seg = expected_packed(padded, lens, cap, -1)
            assert torch.equal(vbuf[vo:vo + cap * esz].cpu(), values.view(torch.uint8)), what
            assert torch.equal(cbuf[co:co + (rows + 1) * 4].cpu().view(torch.int32), cu), what
            assert int(tbuf[to:to + 8].cpu().view(torch.int64)) == total, what
            assert torch.equal(pbuf[po:po + cap * 4].cpu().view(torch.int32), pos), what
            assert torch.equal(sbuf[so:so + cap * 4].cpu().view(torch.int32), seg), what


def test_raw_binding_refuses_bad_arguments():
    from torchkafka_amd.ops import hip

    x = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = x.data_ptr()
    for args in ((p, 3, 2, 2, p, p, 4, 0, p, p, 0, 0),          # element size
                 (p, 8, -1, 2, p, p, 4, 0, p, p, 0, 0),         # rows
                 (p, 8, 2, 2, p, p, 1 << 31, 0, p, p, 0, 0),    # capacity
                 (p, 8, 1 << 20, 1 << 12, p, p, 4, 0, p, p, 0, 0),  # rows * W
                 (p, 8, 2, 2, p, p, 4, 0, 0, p, 0, 0),          # no cu_seqlens
                 (p, 8, 2, 2, p, p, 4, 0, p, p, p, 0)):         # position_ids without segment_ids
        with pytest.raises(ValueError):
            hip().pack_rows(*args, 0)


def test_other_stream_and_repeat_give_the_same_bytes():
    from torchkafka_amd import pack_padded

    rows, W = 257, 9
    lens = _lengths(rows, W, 1)
    padded = _padded(torch.bfloat16, rows, W, 2)
    dev, lens_d = padded.to(DEV), torch.tensor(lens, device=DEV)
    cap = capacities(lens, W)[-1]  # total + 5
    first = pack_padded(dev, lens_d, cap, -1, True)
    again = pack_padded(dev, lens_d, cap, -1, True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = pack_padded(dev, lens_d, cap, -1, True)
    side.synchronize()
    torch.cuda.synchronize()
    check_packed(first, padded, lens, cap, -1, True, "first")
    for name, pb in (("again", again), ("side stream", other)):
        for a, b in zip(first, pb):
            if isinstance(a, torch.Tensor):
                assert torch.equal(bits(a) if a.dim() else a, bits(b) if b.dim() else b), name
            else:
                assert a == b, name
