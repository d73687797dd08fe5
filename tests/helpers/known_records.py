"""Known record contents and plain-torch expected values for the kernel and loader-path tests.

Nothing here calls the package's own references (``reference_fixed`` / ``reference_varlen``, which the
CPU loader also runs): the expected values are written out in plain torch on the CPU, from the bytes
the test produced into the broker.

* ``known_rows``      deterministic source rows: float specials and rounding ties, full-range integers;
* ``produce_known``   one record per row (raw little-endian bytes) into one partition, keys of 0-8 bytes
                      so that the values land at every byte alignment in the log;
* ``norm_vectors``    non-constant per-feature (mean, std): an off-by-one feature index changes the result;
* ``expected_fixed`` / ``expected_varlen``  the documented contract of the loader, inline;
* ``assert_same``     same dtype and shape, same NaN positions, identical bits everywhere else;
* ``assert_within_f32_bound``  a normalised f32 result against a float64 evaluation of (x - mean) / std;
* ``bf16_tie_values`` / ``f16_tie_values`` / ``e4m3_tie_values``  f32 tie and boundary bit patterns.
"""
import random

import torch

FLOATS = (torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn)
_SIGN = -0x80000000  # the f32 sign bit as an int32


def esize(dt: torch.dtype) -> int:
    return torch.empty((), dtype=dt).element_size()


def _f32(bits: torch.Tensor) -> torch.Tensor:
    """int64 bit patterns (0 .. 2^32-1) -> float32."""
    b = bits.to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b >= 1 << 31, b - (1 << 32), b)
    return b.to(torch.int32).view(torch.float32)


def _both_signs(x: torch.Tensor) -> torch.Tensor:
    return torch.cat([x, (x.view(torch.int32) ^ _SIGN).view(torch.float32)])


# ----------------------------------------------------------------------------- rounding ties (bit patterns)
def bf16_tie_values(seed: int = 0, n_upper: int = 4096) -> torch.Tensor:
    """f32 values around every kind of bf16 rounding decision: seeded upper halves plus both ends of
    every binade (mantissa all zeros / all ones, each exponent and sign, zeros, infs and NaNs
    included), each combined with the low halves just below, at and just above the tie."""
    g = torch.Generator().manual_seed(seed)
    upper = torch.randint(0, 1 << 16, (n_upper,), generator=g, dtype=torch.int64)
    exps = torch.arange(256, dtype=torch.int64) << 7
    edges = torch.cat([exps, exps | 0x7F])
    upper = torch.cat([upper, edges, edges | 0x8000])
    low = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)
    return _f32(((upper << 16)[:, None] | low[None, :]).flatten())


def f16_tie_values(seed: int = 0, n_upper: int = 4096) -> torch.Tensor:
    """f32 values around every kind of f16 rounding decision.  Normal range: seeded upper 19 bits with
    the f32 exponent anywhere from below the f16 subnormals (2^-26) to past its overflow (2^16), low
    13 bits just below, at and just above the tie.  Subnormal range (the tie position moves with the
    exponent) and the overflow edge: the midpoint of every pair of adjacent f16 subnormals, and of
    65504 and 65536, with its two f32 neighbours.  Both signs."""
    g = torch.Generator().manual_seed(seed)
    exp = torch.randint(101, 144, (n_upper,), generator=g, dtype=torch.int64)
    man = torch.randint(0, 1 << 10, (n_upper,), generator=g, dtype=torch.int64)
    edge_exp = torch.arange(101, 144, dtype=torch.int64)
    exp = torch.cat([exp, edge_exp, edge_exp])
    man = torch.cat([man, torch.zeros_like(edge_exp), torch.full_like(edge_exp, 0x3FF)])
    upper = (exp << 23) | (man << 13)
    low = torch.tensor([0x0000, 0x0FFF, 0x1000, 0x1001, 0x1FFF], dtype=torch.int64)
    normal = _f32((upper[:, None] | low[None, :]).flatten())
    # subnormals k * 2^-24, k = 0..1024 (1024 is the smallest normal): midpoints (k + 1/2) * 2^-24
    k = torch.arange(0, 1024, dtype=torch.float64)
    mids = torch.cat([(k + 0.5) * 2.0 ** -24, torch.tensor([65520.0, 65504.0, 65536.0], dtype=torch.float64)])
    mids = mids.to(torch.float32)  # exact: at most 12 significant bits
    mb = mids.view(torch.int32).to(torch.int64)
    around = _f32(torch.cat([mb - 1, mb, mb + 1]))
    return _both_signs(torch.cat([normal, around]))


def e4m3_tie_values() -> torch.Tensor:
    """All 256 e4m3fn codes as f32; the midpoint of every pair of adjacent finite codes with its two
    f32 neighbours; the same around 464 (the tie between 448 and the first value that is no longer
    finite), 480 and 2^-10 (half the smallest subnormal).  Both signs."""
    codes = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32)
    finite = codes[:0x7F].to(torch.float64)  # 0 .. 448, ascending
    mids = torch.cat([(finite[:-1] + finite[1:]) / 2, torch.tensor([464.0, 480.0, 2.0 ** -10], dtype=torch.float64)])
    mids = mids.to(torch.float32)  # exact: 5 significant bits at most
    mb = mids.view(torch.int32).to(torch.int64)
    around = _both_signs(_f32(torch.cat([mb - 1, mb, mb + 1])))
    return torch.cat([codes, around])


def special_values() -> torch.Tensor:
    """Hand-picked f32 specials: zeros, infinities, NaN, f32 denormals, fp8 / f16 / bf16 edges."""
    dn = _f32(torch.tensor([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00012345],
                           dtype=torch.int64))
    named = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-42, 448.0, 449.0, 464.0,
                          479.9, 480.0, -464.0, 65504.0, 65520.0, -65520.0, 3.0e38, -3.4e38, 2.0 ** -9, 2.0 ** -10,
                          2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -3.5, 2.0 ** -6,
                          2.0 ** -7 * 1.5, 2.0 ** -14, 2.0 ** -126, 1.0, -1.0, 255.0, 256.5, 257.5])
    return torch.cat([named, dn])


_POOL = {}


def _float_pool() -> torch.Tensor:
    if "f" not in _POOL:
        _POOL["f"] = torch.cat([special_values(), bf16_tie_values(1, 256), f16_tie_values(2, 256),
                                e4m3_tie_values()])
    return _POOL["f"]


def _int_specials(dt: torch.dtype) -> torch.Tensor:
    info = torch.iinfo(dt)
    big = [(1 << 24) + 1, (1 << 24) + 3, (1 << 24) - 1, (1 << 31) - 1, -(1 << 31), (1 << 31), (1 << 32) + 5,
           (1 << 53) + 1, 65504, 65519, 65520, 65536, 448, 449, 464, 480, 255, 256, 257, 127, 128, 129]
    v = [info.min, info.max, 0, 1, info.min + 1, info.max - 1]
    for b in big:
        v += [b, -b]
    if info.min < 0:
        v.append(-1)
    return torch.tensor(sorted({x for x in v if info.min <= x <= info.max}), dtype=torch.int64).to(dt)


# ----------------------------------------------------------------------------- source rows
def known_values(src_dtype: torch.dtype, n: int, seed: int) -> torch.Tensor:
    """``n`` elements of ``src_dtype``, deterministic from ``seed``: the specials first (as many as
    fit), then a seeded mix of specials / ties and values spread over the type's range."""
    g = torch.Generator().manual_seed(seed)
    if src_dtype.is_floating_point:
        pool = _float_pool()
        spread = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
        pick = pool[torch.randint(0, pool.numel(), (n,), generator=g)]
        x = torch.where(torch.rand(n, generator=g) < 0.5, pick, spread)
        sp = special_values()
        k = min(n, sp.numel())
        x[:k] = sp[:k]
        return x.to(src_dtype)
    info = torch.iinfo(src_dtype)
    bits = 8 * esize(src_dtype)
    if bits == 64:
        x = torch.randint(0, 256, (n, 8), generator=g, dtype=torch.int64).to(torch.uint8).view(torch.int64).view(n)
    else:
        x = torch.randint(info.min, info.max + 1, (n,), generator=g, dtype=torch.int64)
    # half of the values at a seeded magnitude: a full-range draw is almost never small
    sh = torch.randint(0, bits, (n,), generator=g, dtype=torch.int64)
    x = torch.where(torch.rand(n, generator=g) < 0.5, x >> sh, x).to(src_dtype)
    sp = _int_specials(src_dtype)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    return x


def known_rows(src_dtype: torch.dtype, shape, n: int, seed: int) -> torch.Tensor:
    """A CPU tensor ``[n, *shape]`` of ``src_dtype``, deterministic from ``seed`` (known_values)."""
    numel = 1
    for d in shape:
        numel *= int(d)
    return known_values(src_dtype, n * numel, seed).view(n, *shape)


def row_bytes(t: torch.Tensor) -> bytes:
    """The raw little-endian bytes of a CPU tensor."""
    return t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()


def produce_known(broker, topic: str, rows, rpb: int, seed: int) -> int:
    """Creates ``topic`` with ONE partition and writes each row's raw bytes as one record value,
    ``rpb`` records per RecordBatch.  Keys are 0-8 bytes long (seeded), so the values land at every
    byte alignment in the log.  One partition (with one worker and ``in_order=True``) makes the
    delivery order the produce order.  Returns the number of records."""
    rng = random.Random(seed)
    vals = [row_bytes(r) for r in rows]
    keys = [b"k" * rng.randrange(0, 9) for _ in vals]
    broker.create_topic(topic, 1)
    for i in range(0, len(vals), rpb):
        broker.produce(topic, vals[i:i + rpb], partition=0, keys=keys[i:i + rpb])
    return len(vals)


# ----------------------------------------------------------------------------- normalisation vectors
def norm_vectors(row: int, seed: int = 0):
    """Per-feature f32 (mean, std) of length ``row``, never constant: no two features share a
    (mean, std) pair (check_norm_vectors), so a wrong feature index changes the result."""
    g = torch.Generator().manual_seed(1000 + seed)
    mean = torch.linspace(-3.0, 3.0, row)[torch.randperm(row, generator=g)].contiguous()
    std = 0.5 + (torch.arange(row) % 7).to(torch.float32) * 0.25
    return mean, std


def check_norm_vectors(mean: torch.Tensor, std: torch.Tensor) -> None:
    row = mean.numel()
    assert mean.dtype == std.dtype == torch.float32 and std.numel() == row
    assert bool((std >= 0.5).all()) and bool(torch.isfinite(mean).all())
    pairs = {(float(m), float(s)) for m, s in zip(mean, std)}
    assert len(pairs) == row, "two features share a (mean, std) pair"
    for i in range(row - 1):
        assert (float(mean[i]), float(std[i])) != (float(mean[i + 1]), float(std[i + 1]))
        assert float(std[i]) != float(std[i + 1])  # an off-by-one index changes the scale for certain


# ----------------------------------------------------------------------------- expected values
def expected_fixed(rows: torch.Tensor, dst: torch.dtype, mean=None, std=None) -> torch.Tensor:
    """What a fixed-width batch must hold: ``rows.to(dst)``, or with normalisation
    ``((x - mean) * (1 / std)).to(dst)`` in f32 per feature (the contract of ``normalize=``)."""
    if mean is None:
        return rows.to(dst)
    n = rows.shape[0]
    x = (rows.to(torch.float32).reshape(n, -1) - mean) * (1.0 / std)
    return x.to(dst).reshape(rows.shape)


def expected_width(lens, pad_to=None, pad_multiple: int = 8, trunc=None) -> int:
    """The documented width of a var-len batch (docs/CONFIG.md): ``pad_to``, else the longest row
    (after the schema's truncation) rounded up to a multiple of ``pad_multiple``."""
    if pad_to is not None:
        return int(pad_to)
    L = max([min(k, trunc) if trunc is not None else k for k in lens], default=0)
    if pad_multiple > 1:
        L = (L + pad_multiple - 1) // pad_multiple * pad_multiple
    return L


def expected_varlen(rows, dst: torch.dtype, L: int, pad=0, trunc=None):
    """(values [n, L], lengths [n] int64, mask [n, L] bool): each row cut to ``trunc`` elements (the
    schema's ``max_len``) and to ``L``, cast with ``Tensor.to`` and written into a tensor pre-filled
    with the pad value (rounded to ``dst`` through f32; integers through int64)."""
    n = len(rows)
    if dst.is_floating_point:
        fill = torch.tensor(float(pad), dtype=torch.float32).to(dst)
    else:
        fill = torch.tensor(int(pad), dtype=torch.int64).to(dst)
    out = fill.repeat(n * L).view(n, L)
    lengths = torch.zeros(n, dtype=torch.int64)
    mask = torch.zeros((n, L), dtype=torch.bool)
    for i, r in enumerate(rows):
        r = r.view(-1)
        if trunc is not None:
            r = r[:trunc]
        k = min(int(r.numel()), L)
        if k:
            out[i, :k] = r[:k].to(dst)
            mask[i, :k] = True
        lengths[i] = k
    return out, lengths, mask


# ----------------------------------------------------------------------------- comparison
def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same(out: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """Same dtype and shape, same NaN positions, identical bits everywhere else."""
    assert out.dtype == ref.dtype and tuple(out.shape) == tuple(ref.shape), (what, out.dtype, ref.dtype,
                                                                             tuple(out.shape), tuple(ref.shape))
    o, r = out.cpu(), ref.cpu()
    if o.dtype.is_floating_point:
        on, rn = torch.isnan(o.float()), torch.isnan(r.float())
        assert torch.equal(on, rn), f"{what}: NaN positions differ at {(on != rn).nonzero()[:8].tolist()}"
        ob, rb = bits(o), bits(r)
        bad = (ob != rb) & ~on
    else:
        bad = o != r
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        got = [o[tuple(i)].item() if not o.dtype.is_floating_point else o[tuple(i)].float().item() for i in idx]
        want = [r[tuple(i)].item() if not r.dtype.is_floating_point else r[tuple(i)].float().item() for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} values differ; first at {idx}: got {got}, want {want}")


def assert_within_f32_bound(out: torch.Tensor, rows: torch.Tensor, mean: torch.Tensor, std: torch.Tensor,
                            what: str = "") -> None:
    """A normalised f32 result against ``(x - mean) / std`` evaluated in float64.  The result comes
    from three correctly rounded f32 operations (the subtraction, the reciprocal of std, the
    product), each within 2^-24 / (1 + 2^-24) relative, and an underflowing product within half an
    f32 denormal: ``|out - exact| <= 3 * 2^-24 * |exact| + 2^-149`` wherever both are finite."""
    assert out.dtype == torch.float32
    n = rows.shape[0]
    o = out.cpu().reshape(n, -1).to(torch.float64)
    exact = (rows.to(torch.float32).reshape(n, -1).to(torch.float64) - mean.to(torch.float64)) / std.to(torch.float64)
    fin = torch.isfinite(o) & torch.isfinite(exact)
    assert bool(fin.any())
    err = (o - exact).abs()
    bound = 3 * 2.0 ** -24 * exact.abs() + 2.0 ** -149
    bad = fin & (err > bound)
    assert not bool(bad.any()), (what, bad.nonzero()[:8].tolist(), err[bad][:8].tolist(), bound[bad][:8].tolist())
