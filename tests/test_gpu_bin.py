"""The gfx950 bin kernels (csrc/hip/bin.hip) and ``bin_padded`` against a Python loop over the rows and
bins (tests/helpers/binned.py): first-fit placement with back-filling, more bins than one 64-bin
ballot step, too few bins (rows left out, later rows still placed), rows cut at seq_len, every
element size, lengths out of range, and -- through the raw binding -- canaries around every output."""
import pytest
import torch

from helpers.binned import binned_layout, check_binned, expected_binned
from helpers.known_records import bits
from helpers.packed import pad_element
from test_gpu_pack import BY_SIZE, _canaried, _intact, _lengths, _padded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = (0, 1, 2, 63, 64, 65, 257, 1025)
WIDTHS = (0, 1, 7, 9)
SEQ_LENS = (1, 5, 9, 12, 64)


def _bin_counts(lens, W: int, seq_len: int, rows: int):
    """default (None), 1, the number the default run used, half of that, rows + 3"""
    used = binned_layout(lens, W, seq_len, rows)["n_bins"]
    return [None] + sorted({1, used, used // 2, rows + 3} - {0})


@pytest.mark.parametrize("rows", ROWS)
def test_bin_padded_matches_the_loop(rows):
    """Up to 65 rows: every width x seq_len x bins x element size.  257 and 1025 rows (more than 64 bins
    in use): every width x seq_len x bins, the element size taking turns."""
    from torchkafka_amd import bin_padded

    turn = 0
    for W in WIDTHS:
        lens = _lengths(rows, W, 31 * rows + W)
        lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
        padded = {esz: _padded(dt, rows, W, rows + W + esz) for esz, dt in BY_SIZE.items()}
        dev = {esz: p.to(DEV) for esz, p in padded.items()}
        for seq_len in SEQ_LENS:
            for bins in _bin_counts(lens, W, seq_len, rows):
                turn += 1
                for esz in (BY_SIZE if rows <= 65 else [list(BY_SIZE)[turn % 4]]):
                    pad = -1 if esz != 4 else float("nan")
                    bb = bin_padded(dev[esz], lens_d, seq_len, bins, pad)
                    assert bb.values.is_cuda and bb.n_bins.is_cuda and bb.cut.is_cuda
                    check_binned(bb, padded[esz], lens, seq_len, rows if bins is None else bins, pad,
                                 f"{rows}x{W} seq_len {seq_len} bins {bins} esz {esz}")
        bb = bin_padded(dev[8], lens_d, 12)  # default bins, pad 0
        check_binned(bb, padded[8], lens, 12, rows, 0, f"{rows}x{W} default")


def test_the_largest_batch_the_device_path_takes():
    from torchkafka_amd import bin_padded
    from torchkafka_amd.ops import hip

    top = int(hip().BIN_MAX_ROWS)
    assert top == 16384
    lens = [1] * top
    lens[5], lens[top - 1] = 0, 0
    padded = _padded(torch.uint8, top, 1, 3)
    bb = bin_padded(padded.to(DEV), torch.tensor(lens, device=DEV), 64, None, -1)  # 256 bins in use of 16384
    check_binned(bb, padded, lens, 64, top, -1, "16384 x 1")
    for rows, bins in ((top + 1, 4), (4, top + 1)):
        x = torch.zeros((rows, 1), dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError):
            bin_padded(x, torch.zeros(rows, dtype=torch.int64, device=DEV), 8, bins)


def test_bin_padded_fp8_and_int32_lengths():
    from torchkafka_amd import bin_padded

    rows, W = 65, 9
    lens = _lengths(rows, W, 5)
    padded = _padded(torch.float8_e4m3fn, rows, W, 9)
    bb = bin_padded(padded.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), 12, None, -1)
    check_binned(bb, padded, lens, 12, rows, -1, "fp8")


def test_bin_padded_takes_a_strided_view():
    from torchkafka_amd import bin_padded

    rows, W = 65, 7
    lens = _lengths(rows, W, 6)
    wide = _padded(torch.int64, rows, W + 3, 4)
    padded = wide[:, 1:W + 1]  # not contiguous
    bb = bin_padded(wide.to(DEV)[:, 1:W + 1], torch.tensor(lens, device=DEV), 12, None, -1)
    check_binned(bb, padded.contiguous(), lens, 12, rows, -1, "strided on the device")


@pytest.mark.parametrize("rows", [5, 65, 257])
def test_lengths_out_of_range_are_clamped(rows):
    from torchkafka_amd import bin_padded

    W = 9
    lens = _lengths(rows, W, 77)
    lens[0], lens[2], lens[-1] = -3, W + 4, W + 4
    padded = _padded(torch.int64, rows, W, 8)
    for seq_len in (5, 12):
        for bins in _bin_counts(lens, W, seq_len, rows):
            bb = bin_padded(padded.to(DEV), torch.tensor(lens, device=DEV), seq_len, bins, -1)
            check_binned(bb, padded, lens, seq_len, rows if bins is None else bins, -1,
                         f"clamped {rows} seq_len {seq_len} bins {bins}")


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("rows,W,seq_len,bad", [(65, 9, 12, False), (65, 9, 5, True), (257, 9, 9, True),
                                                (0, 9, 12, False), (7, 0, 5, False)])
def test_raw_binding_writes_nothing_outside_its_outputs(rows, W, seq_len, bad, off):
    from torchkafka_amd.ops import hip

    lens = _lengths(rows, W, rows + W)
    if bad and rows:
        lens[0], lens[-1] = W + 4, W + 4
        lens[1] = -3
    stream = torch.cuda.current_stream(DEV).cuda_stream
    lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
    for esz, dt in BY_SIZE.items():
        padded = _padded(dt, rows, W, esz + rows)
        dev = padded.to(DEV)
        for bins in _bin_counts(lens, W, seq_len, rows)[1:]:
            cells = bins * seq_len
            outs = {"values": _canaried(cells, esz, off), "segment_ids": _canaried(cells, 4, off),
                    "position_ids": _canaried(cells, 4, off), "bin_lens": _canaried(bins, 4, off),
                    "row_bin": _canaried(rows, 4, off), "row_start": _canaried(rows, 4, off),
                    "row_lens": _canaried(rows, 4, off), "n_bins": _canaried(1, 4, off),
                    "unplaced": _canaried(1, 4, off), "cut": _canaried(1, 8, off)}
            sizes = {"values": cells * esz, "segment_ids": cells * 4, "position_ids": cells * 4, "bin_lens": bins * 4,
                     "row_bin": rows * 4, "row_start": rows * 4, "row_lens": rows * 4, "n_bins": 4, "unplaced": 4,
                     "cut": 8}
            at = {name: buf.data_ptr() + o for name, (buf, o) in outs.items()}
            fill = int(bits(pad_element(dt, -1).reshape(1)).item()) & ((1 << (8 * esz)) - 1)
            hip().bin_rows(dev.data_ptr(), esz, rows, W, lens_d.data_ptr(), seq_len, bins, at["values"], fill,
                           at["segment_ids"], at["position_ids"], at["bin_lens"], at["row_bin"], at["row_start"],
                           at["row_lens"], at["n_bins"], at["unplaced"], at["cut"], stream)
            torch.cuda.synchronize()
            what = f"{rows}x{W} seq_len {seq_len} bins {bins} esz {esz} off {off}"
            got = {}
            for name, (buf, o) in outs.items():
                assert _intact(buf, o, sizes[name]), f"{what}: canary around {name} overwritten"
                got[name] = buf[o:o + sizes[name]].cpu()
            values, seg, pos, lay = expected_binned(padded, lens, seq_len, bins, -1)
            # every cell is written: none still holds the canary unless the expected bytes are the canary's
            assert torch.equal(got["values"], values.contiguous().view(torch.uint8).view(-1)), what
            assert torch.equal(got["segment_ids"].view(torch.int32), seg.view(-1)), what
            assert torch.equal(got["position_ids"].view(torch.int32), pos.view(-1)), what
            for name in ("bin_lens", "row_bin", "row_start", "row_lens"):
                assert got[name].view(torch.int32).tolist() == lay[name], (what, name)
            assert int(got["n_bins"].view(torch.int32)) == lay["n_bins"], what
            assert int(got["unplaced"].view(torch.int32)) == lay["unplaced"], what
            assert int(got["cut"].view(torch.int64)) == lay["cut"], what


def test_raw_binding_refuses_bad_arguments():
    from torchkafka_amd.ops import hip

    x = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = x.data_ptr()
    top = int(hip().BIN_MAX_ROWS)
    # padded, esz, rows, W, lengths, seq_len, bins, values, pad, segment_ids, position_ids, bin_lens, row_bin,
    # row_start, row_lens, n_bins, unplaced, cut
    for args in ((p, 3, 2, 2, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),            # element size
                 (p, 16, 2, 2, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),           # element size
                 (p, 8, -1, 2, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),           # rows
                 (p, 8, 2, -1, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),           # width
                 (p, 8, 2, 2, p, 4, -1, p, 0, p, p, p, p, p, p, p, p, p),           # bins
                 (p, 8, 2, 2, p, 0, 2, p, 0, p, p, p, p, p, p, p, p, p),            # seq_len
                 (p, 8, 2, 2, p, 1 << 30, 2, p, 0, p, p, p, p, p, p, p, p, p),      # bins * seq_len
                 (p, 8, 2, 1 << 30, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),      # rows * W
                 (p, 8, top + 1, 1, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),      # rows above the limit
                 (p, 8, 2, 2, p, 4, top + 1, p, 0, p, p, p, p, p, p, p, p, p),      # bins above the limit
                 (0, 8, 2, 2, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),            # no input
                 (p, 8, 2, 2, 0, 4, 2, p, 0, p, p, p, p, p, p, p, p, p),            # no lengths
                 (p, 8, 2, 2, p, 4, 2, 0, 0, p, p, p, p, p, p, p, p, p),            # no values
                 (p, 8, 2, 2, p, 4, 2, p, 0, p, 0, p, p, p, p, p, p, p),            # no position_ids
                 (p, 8, 2, 2, p, 4, 2, p, 0, p, p, p, 0, p, p, p, p, p),            # no row_bin
                 (p, 8, 2, 2, p, 4, 2, p, 0, p, p, p, p, p, p, p, p, 0)):           # no cut
        with pytest.raises(ValueError):
            hip().bin_rows(*args, 0)


def test_bin_padded_refuses_bad_arguments():
    from torchkafka_amd import bin_padded

    x = torch.zeros((4, 8), dtype=torch.int64, device=DEV)
    n = torch.zeros(4, dtype=torch.int64, device=DEV)
    for seq_len, bins in ((0, None), (-1, None), (8, -1), (1 << 31, None), (1 << 20, 1 << 11)):
        with pytest.raises(ValueError):
            bin_padded(x, n, seq_len, bins)
    with pytest.raises(ValueError):
        bin_padded(x, n[:3], 8)
    with pytest.raises(ValueError):
        bin_padded(x[0], n, 8)


def test_other_stream_and_repeat_give_the_same_bytes():
    from torchkafka_amd import bin_padded

    rows, W, seq_len = 257, 9, 12
    lens = _lengths(rows, W, 1)
    padded = _padded(torch.bfloat16, rows, W, 2)
    dev, lens_d = padded.to(DEV), torch.tensor(lens, device=DEV)
    bins = binned_layout(lens, W, seq_len, rows)["n_bins"] - 5  # some rows are left out
    first = bin_padded(dev, lens_d, seq_len, bins, -1)
    again = bin_padded(dev, lens_d, seq_len, bins, -1)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = bin_padded(dev, lens_d, seq_len, bins, -1)
    side.synchronize()
    torch.cuda.synchronize()
    lay = check_binned(first, padded, lens, seq_len, bins, -1, "first")
    assert lay["unplaced"] > 0
    for name, bb in (("again", again), ("side stream", other)):
        for a, b in zip(first, bb):
            if isinstance(a, torch.Tensor):
                assert torch.equal(bits(a) if a.dim() else a, bits(b) if b.dim() else b), name
            else:
                assert a == b, name
