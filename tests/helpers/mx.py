"""An independent scalar oracle for the MX block-scaled formats, and the blocks the MX tests run on.

The oracle shares nothing with ``reference_mx``: it reads the elements out of the tensor's bytes with
``struct``, walks the blocks and elements in a Python loop, takes the exponent with ``math.frexp`` and
scales with ``math.ldexp`` (exact in double).  e4m3fn rounding is ``Tensor.to(torch.float8_e4m3fn)`` on
the scaled and clamped values (that cast is pinned by tests/test_gpu_kernels.py); e2m1 rounding is a
nearest-neighbour search over the eight magnitudes that prefers the even index on a tie.

``mx_blocks()`` is the table of input blocks ([N, 32] f32, one case per block; ``block_notes()`` names
them), ``table(dtype)`` the same in the input dtype and ``oracle_table(dtype, fmt)`` the oracle's bytes
for it, computed once per process.  A test picks blocks by index: ``pick(idx, dtype, fmt)``.
"""
import functools
import math
import struct

import torch

from helpers.known_records import e4m3_tie_values, known_values, special_values

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = {"f32": F32, "bf16": BF16, "f16": F16}
FORMATS = ("mxfp8", "mxfp4")
EMAX_TOP = {"mxfp8": (8, 448.0), "mxfp4": (2, 6.0)}
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
AMAX_EXPONENTS = (-149, -127, -126, -119, -1, 0, 1, 8, 127)
FLT_MAX = 3.4028234663852886e38


# ----------------------------------------------------------------------------- the oracle
def elements(x: torch.Tensor) -> list:
    """The elements of a CPU f32 / bf16 / f16 tensor as Python floats, read from its bytes."""
    raw = x.contiguous().view(-1).view(torch.uint8).numpy().tobytes()
    n = x.numel()
    if x.dtype == F32:
        return list(struct.unpack(f"<{n}f", raw))
    if x.dtype == F16:
        return list(struct.unpack(f"<{n}e", raw))
    assert x.dtype == BF16
    halves = struct.unpack(f"<{n}H", raw)
    return list(struct.unpack(f"<{n}f", struct.pack(f"<{n}I", *(h << 16 for h in halves))))


def e2m1_code(y: float) -> int:
    a = abs(y)
    idx = min(range(8), key=lambda i: (abs(a - E2M1[i]), i & 1))  # nearest; a tie goes to the even index
    return idx | (8 if math.copysign(1.0, y) < 0 else 0)


def oracle_block(vals: list, fmt: str):
    """32 Python floats -> (scale byte, the block's value bytes: 32 for mxfp8, 16 for mxfp4)."""
    emax, top = EMAX_TOP[fmt]
    assert len(vals) == 32
    n_bytes = 32 if fmt == "mxfp8" else 16
    if any(math.isnan(v) or math.isinf(v) for v in vals):
        return 0xFF, [0] * n_bytes
    amax = max(abs(v) for v in vals)
    E = -127 if amax == 0 else math.frexp(amax)[1] - 1  # amax = m * 2^e, m in [0.5, 1)
    se = max(-127, min(127, E - emax))
    ys = [max(-top, min(top, math.ldexp(v, -se))) for v in vals]
    assert all(abs(y) <= top for y in ys)
    if fmt == "mxfp8":
        out = torch.tensor(ys, dtype=torch.float64).to(F32).to(torch.float8_e4m3fn).view(torch.uint8).tolist()
    else:
        codes = [e2m1_code(y) for y in ys]
        out = [codes[2 * i] | (codes[2 * i + 1] << 4) for i in range(16)]
    return se + 127, out


def oracle_mx(x: torch.Tensor, fmt: str):
    """(values uint8 [n_blocks, 32 | 16], scales uint8 [n_blocks]) of a CPU tensor, block by block."""
    vals = elements(x)
    assert len(vals) % 32 == 0
    scales, out = [], []
    for b in range(0, len(vals), 32):
        s, o = oracle_block(vals[b:b + 32], fmt)
        scales.append(s)
        out.append(o)
    width = 32 if fmt == "mxfp8" else 16
    return (torch.tensor(out, dtype=torch.uint8).view(-1, width), torch.tensor(scales, dtype=torch.uint8))


# ----------------------------------------------------------------------------- the input blocks
def _ulp_below(v: float) -> float:
    b = torch.tensor(v, dtype=F32).view(torch.int32)
    return float((b - 1).view(F32))


def _around(vals) -> torch.Tensor:
    """Each f32 value with its two f32 neighbours, in both signs."""
    t = torch.tensor(list(vals), dtype=F32)
    b = t.view(torch.int32)
    pos = torch.cat([(b - 1).view(F32), t, (b + 1).view(F32)])
    return torch.cat([pos, -pos])


def _anchored(anchor: float, vals: torch.Tensor, notes: list, what: str) -> torch.Tensor:
    """Blocks of 31 values of ``vals`` plus ``anchor`` (which fixes the block's exponent), the anchor at
    a different position in every block."""
    pad = (-vals.numel()) % 31
    vals = torch.cat([vals, torch.zeros(pad)]).view(-1, 31)
    out = torch.empty(vals.shape[0], 32)
    for r in range(vals.shape[0]):
        at = (5 * r + 3) % 32
        out[r] = torch.cat([vals[r, :at], torch.tensor([anchor]), vals[r, at:]])
        notes.append(f"{what} #{r}")
    return out


@functools.lru_cache(maxsize=None)
def _build():
    g = torch.Generator().manual_seed(4107)
    notes, parts = [], []

    def add(block: torch.Tensor, what: str):
        block = block.reshape(-1, 32).to(F32)
        parts.append(block)
        notes.extend(f"{what} #{i}" for i in range(block.shape[0]))

    pool = known_values(F32, 32 * 24, 23)                         # begins with special_values()
    assert torch.equal(pool[:8].view(torch.int32), special_values()[:8].view(torch.int32))
    add(pool, "pool")                                             # blocks with a NaN / Inf are bad blocks
    add(torch.where(torch.isfinite(pool), pool, torch.ones(())), "pool, finite")
    add(torch.zeros(32), "all zero")
    add(-torch.zeros(32), "all -0.0")
    noise = torch.randn(32, generator=g)
    for what, v in (("one NaN", float("nan")), ("one +Inf", float("inf")), ("one -Inf", float("-inf"))):
        blk = noise.clone()
        blk[len(parts) % 32] = v
        add(blk, what)
    # amax = 2^k and one ulp below, the other elements a fixed set of fractions of it (both signs)
    frac = torch.cat([torch.tensor([1.0, -1.0, 0.5, -0.75, 0.0, -0.0, 0.999, 2.0 ** -10]),
                      torch.rand(24, generator=g) * 2 - 1]).to(torch.float64)
    for k in AMAX_EXPONENTS:
        for what, amax in ((f"amax 2^{k}", 2.0 ** k), (f"amax 2^{k} - 1 ulp", _ulp_below(2.0 ** k))):
            add((frac * amax).to(F32).roll(len(parts)), what)
    add((frac * FLT_MAX).to(F32).roll(7), "amax FLT_MAX")
    # se = 0 for mxfp8: the bytes are clamp(+-448) followed by the plain e4m3fn cast
    ties = e4m3_tie_values()
    ties = ties[torch.isfinite(ties) & (ties.abs() < 512)]
    high = torch.tensor([448.0, 449.0, 463.0, 465.0, 479.0, 480.0, 481.0, 496.0, 511.0])
    parts.append(_anchored(256.0, torch.cat([ties, _around(high), _around([464.0])]), notes, "anchored at 256"))
    # se = 0 for mxfp4: every e2m1 midpoint with its neighbours, the grid itself, and the saturated range
    grid = torch.tensor(E2M1)
    fp4 = torch.cat([_around(E2M1_MIDPOINTS), grid, -grid, _around([6.0, 7.0]), torch.tensor([5.5, -5.5, 7.99, -7.99])])
    parts.append(_anchored(4.0, fp4, notes, "anchored at 4"))
    for k in range(-140, 128):                                    # per-block magnitudes
        add(((torch.rand(32, generator=g, dtype=torch.float64) * 2 - 1) * 1.99 * 2.0 ** k).to(F32), f"magnitude 2^{k}")
    blocks = torch.cat(parts)
    assert blocks.shape == (len(notes), 32) and blocks.dtype == F32
    return blocks, tuple(notes)


def mx_blocks() -> torch.Tensor:
    """The table of input blocks, f32 [N, 32].  Do not modify."""
    return _build()[0]


def block_notes() -> tuple:
    """What each block of the table is there for."""
    return _build()[1]


@functools.lru_cache(maxsize=None)
def table(dtype: torch.dtype) -> torch.Tensor:
    """``mx_blocks()`` in the input dtype (a plain cast: an f32 beyond f16's range becomes Inf there
    and its block a bad block, which is one more case).  Do not modify."""
    return mx_blocks().to(dtype)


@functools.lru_cache(maxsize=None)
def oracle_table(dtype: torch.dtype, fmt: str):
    """The oracle's (values [N, 32 | 16], scales [N]) for ``table(dtype)``.  Do not modify."""
    return oracle_mx(table(dtype), fmt)


def pick(idx, dtype: torch.dtype, fmt: str):
    """Blocks ``idx`` of the table -> (x [len(idx), 32] in ``dtype``, values bytes, scale bytes)."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    values, scales = oracle_table(dtype, fmt)
    return table(dtype)[idx], values[idx], scales[idx]


def value_bytes(batch) -> torch.Tensor:
    """An MXBatch's values as CPU uint8, whatever their dtype."""
    return batch.values.cpu().view(torch.uint8)


def assert_mx_equal(batch, values: torch.Tensor, scales: torch.Tensor, what: str = "") -> None:
    """The batch's bytes against expected ``values`` / ``scales`` bytes (any shapes of the same size)."""
    got_s = batch.scales.cpu().reshape(-1)
    want_s = scales.reshape(-1)
    assert batch.scales.dtype == torch.uint8 and got_s.numel() == want_s.numel(), (what, tuple(batch.scales.shape))
    bad = (got_s != want_s).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} scales differ; first at block {bad[:6].tolist()}: got "
                              f"{got_s[bad[:6]].tolist()}, want {want_s[bad[:6]].tolist()}")
    got_v = value_bytes(batch).reshape(-1)
    want_v = values.reshape(-1)
    assert got_v.numel() == want_v.numel(), (what, tuple(batch.values.shape))
    bad = (got_v != want_v).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} value bytes differ; first at byte {bad[:6].tolist()}: got "
                              f"{got_v[bad[:6]].tolist()}, want {want_v[bad[:6]].tolist()}")
