"""The expected binned (first-fit) batch, built by a Python loop over the rows and the bins.

Nothing here calls ``reference_binned`` or the bin kernels: ``binned_layout`` walks the rows one by
one, tries the bins from the lowest up and writes down where every kept element lands,
``expected_binned`` moves the bits.
"""
import torch

from helpers.known_records import assert_same, bits
from helpers.packed import pad_element


def binned_layout(lens, W: int, seq_len: int, bins: int):
    """For rows of ``lens`` elements (clamped to 0..W, cut at seq_len): a dict of plain lists --
    ``row_bin``, ``row_start``, ``row_lens`` per row, ``bin_lens`` per bin, and the counts
    ``n_bins``, ``unplaced``, ``cut``."""
    free = [seq_len] * bins
    row_bin, row_start, row_lens = [], [], []
    unplaced = cut = 0
    for k in lens:
        m = max(0, min(int(k), W))
        n = min(m, seq_len)
        cut += m - n
        row_lens.append(n)
        where = -1
        for b in range(bins):
            if free[b] >= n:
                where = b
                break
        if where < 0:
            row_bin.append(-1)
            row_start.append(-1)
            unplaced += 1
            continue
        row_bin.append(where)
        row_start.append(seq_len - free[where])
        free[where] -= n
    bin_lens = [seq_len - f for f in free]
    return {"row_bin": row_bin, "row_start": row_start, "row_lens": row_lens, "bin_lens": bin_lens,
            "n_bins": sum(1 for k in bin_lens if k > 0), "unplaced": unplaced, "cut": cut}


def expected_binned(padded: torch.Tensor, lens, seq_len: int, bins: int, pad=0):
    """(values [bins, seq_len], segment_ids, position_ids, the ``binned_layout`` dict) of a CPU
    ``padded`` [rows, W]."""
    rows, W = padded.shape
    lay = binned_layout(lens, W, seq_len, bins)
    src = bits(padded.contiguous())
    vals = bits(pad_element(padded.dtype, pad).reshape(1)).repeat(bins * seq_len).view(bins, seq_len)
    seg = torch.full((bins, seq_len), -1, dtype=torch.int32)
    pos = torch.zeros((bins, seq_len), dtype=torch.int32)
    for r in range(rows):
        b, s, n = lay["row_bin"][r], lay["row_start"][r], lay["row_lens"][r]
        if b < 0 or n == 0:
            continue
        vals[b, s:s + n] = src[r, :n]
        seg[b, s:s + n] = r
        pos[b, s:s + n] = torch.arange(n, dtype=torch.int32)
    return vals.view(padded.dtype), seg, pos, lay


def check_binned(bb, padded: torch.Tensor, lens, seq_len: int, bins: int, pad=0, what: str = "",
                 moved: bool = True) -> dict:
    """``bb`` (a BinnedBatch, on any device) against the loop, bit for bit (assert_same); returns the
    expected layout.  ``moved``: ``padded`` is the very tensor that was binned, so NaN payloads of
    the moved elements must survive too; a loader test passes False (see helpers.packed.check_packed)."""
    from torchkafka_amd import BinnedBatch

    assert isinstance(bb, BinnedBatch), (what, type(bb))
    rows = padded.shape[0]
    values, seg, pos, lay = expected_binned(padded, lens, seq_len, bins, pad)
    assert type(bb.seq_len) is int and bb.seq_len == seq_len, (what, bb.seq_len)
    assert_same(bb.values, values, f"{what}: values")
    if moved:
        real = seg >= 0
        assert torch.equal(bits(bb.values.cpu())[real], bits(values)[real]), f"{what}: NaN payloads changed"
    for name, want in (("segment_ids", seg), ("position_ids", pos)):
        got = getattr(bb, name)
        assert got.dtype == torch.int32 and tuple(got.shape) == (bins, seq_len), (what, name, got.dtype, got.shape)
        assert torch.equal(got.cpu(), want), f"{what}: {name}"
    for name, n in (("bin_lens", bins), ("row_bin", rows), ("row_start", rows), ("row_lens", rows)):
        got = getattr(bb, name)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n,), (what, name, got.dtype, got.shape)
        assert got.cpu().tolist() == lay[name], (what, name, got.cpu().tolist()[:16], lay[name][:16])
    for name, dt in (("n_bins", torch.int32), ("unplaced", torch.int32), ("cut", torch.int64)):
        got = getattr(bb, name)
        assert got.dtype == dt and got.dim() == 0, (what, name, got.dtype, got.shape)
        assert int(got) == lay[name], (what, name, int(got), lay[name])
    assert all(k > 0 for k in lay["bin_lens"][:lay["n_bins"]]) and not any(lay["bin_lens"][lay["n_bins"]:]), what
    cut = bb.trim()
    assert isinstance(cut, BinnedBatch) and cut.seq_len == seq_len
    k = lay["n_bins"]
    assert_same(cut.values, values[:k], f"{what}: trim().values")
    assert torch.equal(cut.segment_ids.cpu(), seg[:k]) and torch.equal(cut.position_ids.cpu(), pos[:k]), what
    assert cut.bin_lens.cpu().tolist() == lay["bin_lens"][:k], what
    assert cut.row_bin.cpu().tolist() == lay["row_bin"], what
    return lay
