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


# ----------------------------------------------------------------------------- MX block-scaled formats
MX_FORMATS = {"mxfp8": 0, "mxfp4": 1}   # name -> the kernel's format code
_MX_EMAX_TOP = {"mxfp8": (8, 448.0), "mxfp4": (2, 6.0)}
_MX_SOURCES = (torch.float32, torch.bfloat16, torch.float16)
MX_BLOCK = 32
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _exp2i(e: torch.Tensor) -> torch.Tensor:
    """``2.0 ** e`` as exact f32 for an integer tensor ``e`` in [-126, 127], built from its bits."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


class MXBatch(NamedTuple):
    """A tensor in an OCP Microscaling (MX v1.0) format: blocks of 32 consecutive elements of the last
    dimension share one power-of-two scale (``quantize_mx``, ``DeviceLoader(quantize=...)``).

    Fields:
        values: ``"mxfp8"``: ``float8_e4m3fn`` in the input's shape.  ``"mxfp4"``: ``uint8`` with the last
            dimension halved, two e2m1 codes per byte -- element ``2i`` in the low nibble, ``2i + 1`` in
            the high one (torch's ``float4_e2m1fn_x2`` convention); a code is ``sign << 3 | index`` into
            the magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6.
        scales: ``uint8`` E8M0 bytes in the input's shape with the last dimension ``/ 32``, plain
            row-major: block ``b`` of a row stands for ``2 ** (scales[..., b] - 127)`` times its elements;
            0xFF marks a block that held a NaN or an infinity (it dequantises to NaN, its element bytes
            are 0).  The pre-swizzled scale layouts that particular GEMM libraries want are out of
            scope: permute ``scales`` yourself.
        fmt: ``"mxfp8"`` or ``"mxfp4"``.
    """

    values: torch.Tensor
    scales: torch.Tensor
    fmt: str

    @property
    def scales_e8m0(self) -> torch.Tensor:
        """``scales`` viewed as ``torch.float8_e8m0fnu`` (no copy)."""
        return self.scales.view(torch.float8_e8m0fnu)

    @property
    def values_fp4x2(self) -> torch.Tensor:
        """mxfp4 ``values`` viewed as ``torch.float4_e2m1fn_x2`` (no copy)."""
        if self.fmt != "mxfp4":
            raise TypeError(f"values_fp4x2: the batch is {self.fmt}, not mxfp4")
        return self.values.view(torch.float4_e2m1fn_x2)

    def dequantize(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """The values the batch stands for, in the input's shape: plain torch on the batch's device,
        integer arithmetic on the scale bytes and exact power-of-two scaling (no arithmetic on
        ``float8_e8m0fnu`` / ``float4_e2m1fn_x2`` tensors)."""
        if self.fmt == "mxfp8":
            v = self.values.to(torch.float32)
        else:
            lut = torch.tensor(_E2M1 + tuple(-m for m in _E2M1), dtype=torch.float32, device=self.values.device)
            codes = torch.stack([self.values & 0xF, self.values >> 4], dim=-1)
            v = lut[codes.to(torch.int64)].flatten(-2)
        shape = v.shape
        e = self.scales.to(torch.int32) - 127                    # [-127, 127]; 128: the NaN scale
        nan = (e == 128).unsqueeze(-1)
        e = e.clamp(max=127)
        lo = e >> 1                                              # 2^e = 2^lo * 2^(e - lo), both factors normal
        v = v.reshape(*self.scales.shape, MX_BLOCK) * _exp2i(lo).unsqueeze(-1) * _exp2i(e - lo).unsqueeze(-1)
        v = torch.where(nan, torch.full_like(v, float("nan")), v)
        return v.reshape(shape).to(dtype)


def _mx_check(x: torch.Tensor, fmt: str) -> None:
    if fmt not in MX_FORMATS:
        raise ValueError(f"mx: fmt must be 'mxfp8' or 'mxfp4', not {fmt!r}")
    if not isinstance(x, torch.Tensor) or x.dtype not in _MX_SOURCES:
        got = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
        raise TypeError(f"mx: the input must be a float32, bfloat16 or float16 tensor, not {got}")
    if x.dim() < 1 or x.shape[-1] % MX_BLOCK:
        raise ValueError(f"mx: the last dimension must be a multiple of {MX_BLOCK}, got shape {tuple(x.shape)}")
    if x.numel() >= _PACK_LIMIT:
        raise ValueError("mx: numel must be below 2^31")


def mx_launch(x: torch.Tensor, code: int, fmt: str) -> MXBatch:
    """The quantise kernel on the current stream; ``x`` contiguous f32 / bf16 / f16 on the GPU with
    ``shape[-1] % 32 == 0`` (the loader's per-batch entry: no checks).  The kernel loads 16 bytes per
    lane: a view that starts off a 16-byte boundary is copied first."""
    if x.data_ptr() % 16:
        x = x.clone()
    values, scales = hip().mx_tensors(x, code)  # allocates the outputs natively
    return MXBatch(values, scales, fmt)


def quantize_mx(x: torch.Tensor, fmt: str = "mxfp8") -> MXBatch:
    """``x`` (float32, bfloat16 or float16; last dimension a multiple of 32; ``numel < 2^31``) ->
    :class:`MXBatch`, in one gfx950 launch on the current stream (csrc/hip/mx_quant.hip).  Per block
    of 32: the scale is ``2 ** (floor(log2(amax)) - emax)`` (emax 8 / 2, the exponent clamped to
    [-127, 127]), each element is ``x / scale`` saturated to +-448 / +-6 and rounded to nearest even;
    a block with a NaN or an infinity gets the NaN scale 0xFF and zero elements.  A non-contiguous
    input is made contiguous.  CPU tensors take :func:`reference_mx`."""
    _mx_check(x, fmt)
    if x.device.type != "cuda":
        return reference_mx(x, fmt)
    return mx_launch(x.contiguous(), MX_FORMATS[fmt], fmt)


# ----------------------------------------------------------------------------- struct records
def _struct_check(raw: torch.Tensor, schema) -> torch.Tensor:
    size = schema.size
    if not isinstance(raw, torch.Tensor) or raw.dim() != 2 or not (
            (raw.dtype == torch.int32 and raw.shape[1] * 4 == size) or
            (raw.dtype == torch.uint8 and raw.shape[1] == size)):
        got = (raw.dtype, tuple(raw.shape)) if isinstance(raw, torch.Tensor) else type(raw).__name__
        raise ValueError(f"struct: raw must be int32 [rows, {size // 4}] or uint8 [rows, {size}], got {got}")
    if not raw.is_contiguous():
        raise ValueError("struct: raw must be contiguous")
    if raw.shape[0] * size >= _PACK_LIMIT:
        raise ValueError("struct: rows * size must be below 2^31")
    return raw


def struct_launch(raw: torch.Tensor, schema) -> dict:
    """The split kernel on the current stream; ``raw`` a contiguous device batch of ``schema``'s
    carrier with at least one row (the loader's per-batch entry: no checks).  The kernel reads
    dwords: a view that starts off a 4-byte boundary is copied first."""
    if raw.data_ptr() % 4:
        raw = raw.clone()
    outs = hip().struct_tensors(raw, schema.size, schema.device_spec(raw.device))  # allocates the outputs natively
    return {f.name: t for f, t in zip(schema.members, outs)}


def split_struct(raw: torch.Tensor, schema) -> dict:
    """A batch of :class:`~torchkafka_amd.Struct` records -- contiguous int32 ``[rows, size // 4]``
    (the delivered carrier) or uint8 ``[rows, size]`` -- -> ``{field name: tensor [rows, *shape]}``
    with every field's ``out`` and ``normalize`` applied, in one gfx950 launch on the current stream
    (csrc/hip/struct_split.hip) whatever the number of fields.  ``rows == 0`` makes no launch.  CPU
    tensors take :func:`reference_struct`."""
    _struct_check(raw, schema)
    if raw.device.type != "cuda":
        return reference_struct(raw, schema)
    if raw.shape[0] == 0:
        return {f.name: torch.empty((0, *f.shape), dtype=f.out_dtype, device=raw.device) for f in schema.members}
    return struct_launch(raw, schema)


# ----------------------------------------------------------------------------- torch references
def reference_struct(raw: torch.Tensor, schema) -> dict:
    """:func:`split_struct` in plain torch, on any device (the CPU loader's path), bit for bit: per
    field a copy of its byte slice viewed as ``dtype``, ``.to(out)`` and the normalise step."""
    _struct_check(raw, schema)
    rows = raw.shape[0]
    by = raw.view(torch.uint8)
    out = {}
    for f, off in zip(schema.members, schema.offsets):
        # a fresh dense copy, not contiguous(): a one-row slice already counts as contiguous and would
        # keep its odd offset and the record's stride
        x = by[:, off:off + f.nbytes].clone(memory_format=torch.contiguous_format).view(f.dtype).view(rows, *f.shape)
        out[f.name] = f.convert(x)
    return out


def reference_mx(x: torch.Tensor, fmt: str = "mxfp8") -> MXBatch:
    """:func:`quantize_mx` in plain torch, on any device (the CPU path), byte for byte."""
    _mx_check(x, fmt)
    emax, top = _MX_EMAX_TOP[fmt]
    K = x.shape[-1]
    blk = x.contiguous().to(torch.float32).reshape(-1, MX_BLOCK)  # bf16 / f16 widen exactly
    mag = blk.view(torch.int32) & 0x7FFFFFFF
    amax = mag.max(dim=1).values if blk.shape[0] else mag.new_zeros(0)  # orders |v|; NaN and Inf on top
    bad = amax >= 0x7F800000
    se = ((amax >> 23) - 127 - emax).clamp(min=-127)             # a zero or subnormal amax: field 0, clamps
    # ldexp(v, -se) as one exact multiply: 2^-se is a normal f32 for every -se in [-125, 127]
    y = (blk * _exp2i(-se).unsqueeze(1)).clamp(-top, top)
    y = torch.where(bad.unsqueeze(1), torch.zeros_like(y), y)    # (keeps NaN out of the encoders)
    if fmt == "mxfp8":
        codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        a = y.abs()
        idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
        codes = idx | (torch.signbit(y).to(torch.uint8) << 3)    # midpoints went to the even index above
    codes = torch.where(bad.unsqueeze(1), torch.zeros_like(codes), codes)
    scales = torch.where(bad, torch.full_like(se, 255), se + 127).to(torch.uint8).reshape(*x.shape[:-1], K // MX_BLOCK)
    if fmt == "mxfp8":
        return MXBatch(codes.view(torch.float8_e4m3fn).reshape(x.shape), scales, fmt)
    pairs = codes.reshape(-1, 2)
    return MXBatch((pairs[:, 0] | (pairs[:, 1] << 4)).reshape(*x.shape[:-1], K // 2), scales, fmt)


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
