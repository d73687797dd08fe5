"""Batch collate on device (gfx950 HIP kernels) and the matching torch references.

Standalone entry points on device tensors (used by tests and by users who
already hold CSR/dense batches on the GPU); the DeviceLoader drives the same
kernels through the H2D engine on its pinned staging buffers.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .native import hip

DTYPE_CODE = {
    torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float8_e4m3fn: 3, torch.uint8: 4,
    torch.int8: 5, torch.int32: 6, torch.int64: 7,
}
CODE_DTYPE = {v: k for k, v in DTYPE_CODE.items()}
FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn)


def _code(dt: torch.dtype) -> int:
    try:
        return DTYPE_CODE[dt]
    except KeyError:
        raise TypeError(f"collate: unsupported dtype {dt}") from None


def _stream_ptr(device: torch.device) -> int:
    # the raw handle: ~0.08 µs, against ~1.9 µs for torch.cuda.current_stream(device).cuda_stream
    # (host_overhead.log), which builds a Stream object per call
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def normalize_params(normalize, row: int, device) -> tuple[torch.Tensor, torch.Tensor] | None:
    """(mean, std) -> device (shift, scale) f32 vectors of length ``row`` (scale = 1/std)."""
    if normalize is None:
        return None
    mean, std = normalize
    mean = torch.as_tensor(mean, dtype=torch.float32).flatten()
    std = torch.as_tensor(std, dtype=torch.float32).flatten()
    mean = mean.expand(row) if mean.numel() == 1 else mean
    std = std.expand(row) if std.numel() == 1 else std
    if mean.numel() != row or std.numel() != row:
        raise ValueError(f"normalize mean/std must have 1 or {row} elements")
    return mean.contiguous().to(device), (1.0 / std).contiguous().to(device)


def collate_fixed(src: torch.Tensor, dtype: torch.dtype, normalize=None) -> torch.Tensor:
    """Casts a dense ``[rows, *shape]`` device batch to ``dtype`` with optional fused (x-mean)/std."""
    if src.device.type != "cuda":
        return reference_fixed(src, dtype, normalize)
    src = src.contiguous()
    rows = src.shape[0]
    row = src[0].numel() if rows else 0
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    prm = normalize_params(normalize, row, src.device)
    shift, scale = (prm[0].data_ptr(), prm[1].data_ptr()) if prm is not None else (0, 0)
    hip().collate_fixed(src.data_ptr(), _code(src.dtype), out.data_ptr(), _code(dtype), rows, row, shift, scale,
                        _stream_ptr(src.device))
    return out


def collate_varlen(offsets: torch.Tensor, values: torch.Tensor, dtype: torch.dtype, L: int | None = None,
                   pad_value: float = 0, return_mask: bool = False):
    """CSR (``offsets`` int32 [rows+1], ``values`` [nnz]) -> padded ``[rows, L]`` + lengths (+ mask)."""
    rows = offsets.numel() - 1
    lens = offsets[1:] - offsets[:-1]
    if L is None:
        L = int(lens.max().item()) if rows else 0
    if values.device.type != "cuda":
        return reference_varlen(offsets, values, dtype, L, pad_value, return_mask)
    if offsets.dtype != torch.int32:
        raise TypeError("offsets must be int32")
    dev = values.device
    # the kernel stages 16-byte aligned windows: give it an aligned copy with slack
    esz = values.element_size()
    buf = torch.zeros(values.numel() * esz + 64, dtype=torch.uint8, device=dev)
    buf[: values.numel() * esz].copy_(values.contiguous().view(torch.uint8).flatten())
    out = torch.empty((rows, L), dtype=dtype, device=dev)
    lengths = torch.empty(rows, dtype=torch.int64, device=dev)
    mask = torch.empty((rows, L), dtype=torch.bool, device=dev) if return_mask else None
    hip().collate_varlen(offsets.contiguous().data_ptr(), buf.data_ptr(), _code(values.dtype), out.data_ptr(),
                         _code(dtype), rows, L, float(pad_value), lengths.data_ptr(),
                         mask.data_ptr() if mask is not None else 0, _stream_ptr(dev))
    return (out, lengths, mask) if return_mask else (out, lengths)


# ----------------------------------------------------------------------------- packed (cu_seqlens) layout
class PackedBatch(NamedTuple):
    """A var-len batch without padding between its rows (``layout="packed"``).

    ``values[cu_seqlens[r]:cu_seqlens[r + 1]]`` is row ``r``; elements from ``cu_seqlens[-1]`` up to
    the capacity ``values.numel()`` hold the pad value.

    Fields:
        values: 1-D ``[capacity]`` in the output dtype.
        cu_seqlens: int32 ``[rows + 1]``, ``cu_seqlens[0] == 0``, clamped to the capacity: a row that
            does not fit is cut there and the rows after it are empty.
        max_seqlen: the width ``W`` of the padded batch this was packed from -- an upper BOUND on the
            longest row (exact only with ``pad_to=None, pad_multiple=1``).
        total: 0-dim int64 device tensor, the unclamped sum of the lengths; ``total > capacity``
            means rows were cut.  Reading it synchronises, so the loader never does.
        position_ids: int32 ``[capacity]`` (``return_ids=True``): ``i`` for element ``i`` of its row, 0 in the tail.
        segment_ids: int32 ``[capacity]`` (``return_ids=True``): the row index, -1 in the tail.
    """

    values: torch.Tensor
    cu_seqlens: torch.Tensor
    max_seqlen: int
    total: torch.Tensor
    position_ids: torch.Tensor | None = None
    segment_ids: torch.Tensor | None = None

    def trim(self) -> torch.Tensor:
        """``values[:min(total, capacity)]``: the real elements only.  SYNCHRONISES with the device
        (it reads ``total``); keep the fixed-capacity ``values`` where shapes must stay static."""
        return self.values[:min(int(self.total.item()), self.values.numel())]


_BITS_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_PACK_LIMIT = 1 << 31  # cu_seqlens is int32


def pad_fill(dtype: torch.dtype, pad_value: float = 0) -> torch.Tensor:
    """``pad_value`` as one CPU element of ``dtype``, rounded as the padded path rounds it (floats
    through f32, integers through int64)."""
    if dtype in FLOAT_DTYPES:
        return torch.tensor(float(pad_value), dtype=torch.float32).to(dtype)
    return torch.tensor(int(pad_value), dtype=torch.int64).to(dtype)


def pad_bits(dtype: torch.dtype, pad_value: float = 0) -> int:
    """The bit pattern of :func:`pad_fill` as an unsigned int (what the pack kernel stores)."""
    fill = pad_fill(dtype, pad_value)
    esz = fill.element_size()
    return int(fill.view(_BITS_VIEW[esz]).item()) & ((1 << (8 * esz)) - 1)


def _pack_capacity(padded: torch.Tensor, lengths: torch.Tensor, capacity) -> tuple[int, int, int]:
    if padded.dim() != 2:
        raise ValueError("pack: padded must be [rows, width]")
    rows, W = padded.shape
    if lengths.dim() != 1 or lengths.numel() != rows:
        raise ValueError("pack: lengths must be [rows]")
    if padded.element_size() not in _BITS_VIEW:
        raise TypeError(f"pack: unsupported dtype {padded.dtype}")
    cap = rows * W if capacity is None else int(capacity)
    if cap < 0 or cap >= _PACK_LIMIT or rows * W >= _PACK_LIMIT:
        raise ValueError("pack: capacity and rows * width must be in [0, 2^31)")
    return rows, W, cap


def pack_launch(padded: torch.Tensor, lengths: torch.Tensor, cap: int, bits: int, return_ids: bool) -> PackedBatch:
    """The pack kernel on the current stream; ``padded`` contiguous ``[rows, W]`` on the GPU,
    ``lengths`` contiguous int64, ``bits`` from :func:`pad_bits` (the loader's per-batch entry: no checks)."""
    out = hip().pack_tensors(padded, lengths, cap, bits, return_ids)  # allocates the outputs natively
    if return_ids:
        return PackedBatch(out[0], out[1], padded.shape[1], out[2], out[3], out[4])
    return PackedBatch(out[0], out[1], padded.shape[1], out[2])


def pack_padded(padded: torch.Tensor, lengths: torch.Tensor, capacity: int | None = None, pad_value: float = 0,
                return_ids: bool = False) -> PackedBatch:
    """Padded ``[rows, W]`` + ``lengths`` [rows] -> :class:`PackedBatch` of ``capacity`` elements
    (default ``rows * W``: nothing is ever cut), in one gfx950 launch on the current stream (two above
    ``hip().PACK_FUSED_ROWS`` rows).  A length below 0 counts as 0, one above ``W`` as ``W``.  CPU
    tensors take :func:`reference_packed`."""
    if padded.device.type != "cuda":
        return reference_packed(padded, lengths, capacity, pad_value, return_ids)
    rows, W, cap = _pack_capacity(padded, lengths, capacity)
    lengths = lengths.to(device=padded.device, dtype=torch.int64).contiguous()
    return pack_launch(padded.contiguous(), lengths, cap, pad_bits(padded.dtype, pad_value), return_ids)


# ----------------------------------------------------------------------------- binned (first-fit) layout
class BinnedBatch(NamedTuple):
    """A var-len batch with several rows packed into each fixed-length sequence (``layout="binned"``).

    Rows are placed first-fit in arrival order: row ``r`` goes to the lowest of the ``bins`` sequences
    that still has room for it and lies at ``values[row_bin[r], row_start[r]:row_start[r] + row_lens[r]]``.
    A row longer than ``seq_len`` is cut there; a row that fits no bin is left out (``row_bin == -1``).
    The bins in use are a prefix, ``[0, n_bins)``.

    Fields:
        values: ``[bins, seq_len]`` in the output dtype, the pad value where no row landed.
        segment_ids: int32 ``[bins, seq_len]``: the row's index within the batch, -1 in padding.
        position_ids: int32 ``[bins, seq_len]``: ``i`` for element ``i`` of its row, 0 in padding.
        bin_lens: int32 ``[bins]``, the elements placed in each bin.
        row_bin, row_start: int32 ``[rows]``, where each row went (-1 / -1: it fitted no bin).
        row_lens: int32 ``[rows]``, each row's length after the cut at ``seq_len``.
        n_bins: 0-dim int32 device tensor, the number of bins holding an element.
        unplaced: 0-dim int32 device tensor, the rows that fitted no bin.
        cut: 0-dim int64 device tensor, the elements cut off rows longer than ``seq_len``.
            ``unplaced > 0`` or ``cut > 0`` shows an overflow; reading them synchronises, so the
            loader never does.
        seq_len: the length of every sequence (a Python int).

    On the GPU ``segment_ids`` / ``position_ids`` are the two planes of one allocation, and the int32
    metadata tensors are slices of another.
    """

    values: torch.Tensor
    segment_ids: torch.Tensor
    position_ids: torch.Tensor
    bin_lens: torch.Tensor
    row_bin: torch.Tensor
    row_start: torch.Tensor
    row_lens: torch.Tensor
    n_bins: torch.Tensor
    unplaced: torch.Tensor
    cut: torch.Tensor
    seq_len: int

    def trim(self) -> "BinnedBatch":
        """The batch restricted to the bins in use: ``values``, ``segment_ids``, ``position_ids`` and
        ``bin_lens`` cut to ``[:n_bins]``.  SYNCHRONISES with the device (it reads ``n_bins``); keep
        the full ``[bins, seq_len]`` tensors where shapes must stay static."""
        k = int(self.n_bins.item())
        return self._replace(values=self.values[:k], segment_ids=self.segment_ids[:k],
                             position_ids=self.position_ids[:k], bin_lens=self.bin_lens[:k])


def _bin_shape(padded: torch.Tensor, lengths: torch.Tensor, seq_len, bins) -> tuple[int, int, int, int]:
    if padded.dim() != 2:
        raise ValueError("bin: padded must be [rows, width]")
    rows, W = padded.shape
    if lengths.dim() != 1 or lengths.numel() != rows:
        raise ValueError("bin: lengths must be [rows]")
    if padded.element_size() not in _BITS_VIEW:
        raise TypeError(f"bin: unsupported dtype {padded.dtype}")
    seq_len = int(seq_len)
    bins = rows if bins is None else int(bins)
    if seq_len < 1 or bins < 0:
        raise ValueError("bin: seq_len must be >= 1 and bins >= 0")
    if seq_len >= _PACK_LIMIT or bins * seq_len >= _PACK_LIMIT or rows * W >= _PACK_LIMIT:
        raise ValueError("bin: rows * width and bins * seq_len must be below 2^31")
    return rows, W, seq_len, bins


def bin_launch(padded: torch.Tensor, lengths: torch.Tensor, seq_len: int, bins: int, bits: int) -> BinnedBatch:
    """The bin kernels on the current stream; ``padded`` contiguous ``[rows, W]`` on the GPU,
    ``lengths`` contiguous int64, ``bits`` from :func:`pad_bits` (the loader's per-batch entry)."""
    return BinnedBatch(*hip().bin_tensors(padded, lengths, seq_len, bins, bits), seq_len)


def bin_padded(padded: torch.Tensor, lengths: torch.Tensor, seq_len: int, bins: int | None = None,
               pad_value: float = 0) -> BinnedBatch:
    """Padded ``[rows, W]`` + ``lengths`` [rows] -> :class:`BinnedBatch` of ``bins`` sequences of
    ``seq_len`` elements (default ``bins = rows``: every row finds a bin), rows placed first-fit in
    arrival order, in two gfx950 launches on the current stream.  A length below 0 counts as 0, one
    above ``W`` as ``W``.  ``rows`` and ``bins`` may be at most ``hip().BIN_MAX_ROWS`` on the GPU
    (``ValueError`` above); CPU tensors take :func:`reference_binned`, which has no such limit."""
    if padded.device.type != "cuda":
        return reference_binned(padded, lengths, seq_len, bins, pad_value)
    rows, W, seq_len, bins = _bin_shape(padded, lengths, seq_len, bins)
    limit = int(hip().BIN_MAX_ROWS)
    if rows > limit or bins > limit:
        raise ValueError(f"bin: the device path takes at most {limit} rows and bins")
    lengths = lengths.to(device=padded.device, dtype=torch.int64).contiguous()
    return bin_launch(padded.contiguous(), lengths, seq_len, bins, pad_bits(padded.dtype, pad_value))


# ----------------------------------------------------------------------------- torch references
def reference_fixed(src: torch.Tensor, dtype: torch.dtype, normalize=None) -> torch.Tensor:
    if normalize is None:
        return src.to(dtype)
    row = src[0].numel() if src.shape[0] else 0
    prm = normalize_params(normalize, row, src.device)
    x = src.reshape(src.shape[0], -1).to(torch.float32)
    x = (x - prm[0]) * prm[1]
    return x.to(dtype).reshape(src.shape)


def reference_varlen(offsets: torch.Tensor, values: torch.Tensor, dtype: torch.dtype, L: int,
                     pad_value: float = 0, return_mask: bool = False):
    rows = offsets.numel() - 1
    offs = offsets.to(torch.int64).cpu()
    lens = (offs[1:] - offs[:-1]).clamp(max=L)
    if dtype in FLOAT_DTYPES:
        out = torch.full((rows, L), float(pad_value), dtype=torch.float32, device=values.device).to(dtype)
    else:
        out = torch.full((rows, L), int(pad_value), dtype=torch.int64, device=values.device).to(dtype)
    if rows and int(lens.sum()):
        # vectorised scatter (no per-row Python loop): element j of row r lands at out[r, j]
        dev = values.device
        lens_d, starts = lens.to(dev), offs[:-1].to(dev)
        row_idx = torch.repeat_interleave(torch.arange(rows, device=dev), lens_d)
        first = torch.cumsum(lens_d, 0) - lens_d  # position of each row's first element in the gather
        col_idx = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(first, lens_d)
        src_idx = torch.repeat_interleave(starts, lens_d) + col_idx
        out[row_idx, col_idx] = values[src_idx].to(dtype)
    lengths = lens.to(values.device)
    if return_mask:
        mask = torch.arange(L, device=values.device)[None, :] < lengths[:, None]
        return out, lengths, mask
    return out, lengths


def reference_packed(padded: torch.Tensor, lengths: torch.Tensor, capacity: int | None = None, pad_value: float = 0,
                     return_ids: bool = False) -> PackedBatch:
    """:func:`pack_padded` in plain torch (the CPU path).  Works on integer views of the element
    size, so fp8 values and NaN payloads pass through untouched."""
    rows, W, cap = _pack_capacity(padded, lengths, capacity)
    dev = padded.device
    ib = _BITS_VIEW[padded.element_size()]
    src = padded.contiguous().view(ib)
    lens = lengths.to(device=dev, dtype=torch.int64).clamp(0, W)
    ends = torch.cumsum(lens, 0)  # int64
    total = ends[-1].clone() if rows else torch.zeros((), dtype=torch.int64, device=dev)
    cu = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    cu[1:] = ends.clamp(max=cap)
    kept_per_row = cu[1:] - cu[:-1]
    kept = int(cu[-1])
    values = torch.full((cap,), int(pad_fill(padded.dtype, pad_value).view(ib).item()), dtype=ib, device=dev)
    row_idx = torch.repeat_interleave(torch.arange(rows, device=dev), kept_per_row)
    col_idx = torch.arange(kept, device=dev) - torch.repeat_interleave(cu[:-1], kept_per_row)
    values[:kept] = src[row_idx, col_idx]
    pos = seg = None
    if return_ids:
        pos = torch.zeros(cap, dtype=torch.int32, device=dev)
        seg = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        pos[:kept] = col_idx.to(torch.int32)
        seg[:kept] = row_idx.to(torch.int32)
    return PackedBatch(values.view(padded.dtype), cu.to(torch.int32), W, total, pos, seg)


def reference_binned(padded: torch.Tensor, lengths: torch.Tensor, seq_len: int, bins: int | None = None,
                     pad_value: float = 0) -> BinnedBatch:
    """:func:`bin_padded` in plain torch (the CPU path; no size limit).  The placement walks the rows
    in order -- first-fit is sequential -- and searches the bins with one torch op per row; the
    elements then move in one gather over integer views of the element size, so fp8 values and NaN
    payloads pass through untouched."""
    rows, W, seq_len, bins = _bin_shape(padded, lengths, seq_len, bins)
    dev = padded.device
    ib = _BITS_VIEW[padded.element_size()]
    src = padded.contiguous().view(ib)
    full = lengths.to(device="cpu", dtype=torch.int64).clamp(0, W)
    lens = full.clamp(max=seq_len)
    room = torch.full((bins,), seq_len, dtype=torch.int64)
    row_bin = torch.full((rows,), -1, dtype=torch.int64)
    row_start = torch.full((rows,), -1, dtype=torch.int64)
    for r, n in enumerate(lens.tolist()):
        fits = torch.nonzero(room >= n)
        if fits.numel():
            b = int(fits[0])
            row_bin[r], row_start[r] = b, seq_len - int(room[b])
            room[b] -= n
    placed = row_bin >= 0
    kept_per_row = torch.where(placed, lens, torch.zeros_like(lens))
    kept = int(kept_per_row.sum())
    row_idx = torch.repeat_interleave(torch.arange(rows), kept_per_row)
    col_idx = torch.arange(kept) - torch.repeat_interleave(torch.cumsum(kept_per_row, 0) - kept_per_row, kept_per_row)
    cell = (row_bin[row_idx] * seq_len + row_start[row_idx] + col_idx).to(dev)
    row_idx, col_idx = row_idx.to(dev), col_idx.to(dev)
    values = torch.full((bins * seq_len,), int(pad_fill(padded.dtype, pad_value).view(ib).item()), dtype=ib, device=dev)
    seg = torch.full((bins * seq_len,), -1, dtype=torch.int32, device=dev)
    pos = torch.zeros(bins * seq_len, dtype=torch.int32, device=dev)
    values[cell] = src[row_idx, col_idx]
    seg[cell] = row_idx.to(torch.int32)
    pos[cell] = col_idx.to(torch.int32)
    bin_lens = seq_len - room

    def i32(t):
        return t.to(device=dev, dtype=torch.int32)

    return BinnedBatch(values.view(padded.dtype).view(bins, seq_len), seg.view(bins, seq_len), pos.view(bins, seq_len),
                       i32(bin_lens), i32(row_bin), i32(row_start), i32(lens), i32((bin_lens > 0).sum()),
                       i32((~placed).sum()), (full - lens).sum().to(dev), seq_len)
