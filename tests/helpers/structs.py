"""The oracle of the Struct schema tests: a Python loop over rows and fields, independent of
``reference_struct`` / ``Field.convert``.

A field of a record is the bytes ``row[off : off + n]`` copied into a fresh ``bytearray`` (so
``torch.frombuffer`` sees aligned memory).  With ``out=None`` and no ``normalize`` those bytes are
the result.  Otherwise: a float destination gets ``frombuffer(dtype).to(float32)``, the affine step
``(x - mean) * (1 / std)`` in float32, and one ``.to(out)``; an integer destination gets
``frombuffer(dtype).to(out)`` (an int64 does not survive a detour through float32, and ``Conv``
takes none).

Comparison: identity fields and integer outputs by bytes; converted float outputs by NaN positions,
then bytes everywhere else.
"""
import math
import struct as pystruct

import torch

F32, F16, BF16, FP8 = torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn
U8, I8, I32, I64 = torch.uint8, torch.int8, torch.int32, torch.int64
SOURCES = (F32, F16, BF16, U8, I8, I32, I64)
OUTS = (F32, F16, BF16, FP8, I32, I64)
FLOATS = (F32, F16, BF16, FP8)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

# ±0, ±inf, NaN, subnormals, 448 and just above it (e4m3fn's top and its NaN threshold 464 / 480),
# 65504 and just above it (f16's top and the 65520 tie to inf)
SPECIALS_F32 = [0.0, -0.0, math.inf, -math.inf, math.nan, 1e-45, -1e-45, 1e-40, 5.9e-8, 6.1e-5, 448.0, 448.5, 464.0,
                464.5, 480.0, -448.0, -465.0, 65504.0, 65519.9, 65520.0, 65536.0, -65520.0, 0.001953125, 0.0009765625,
                1.0, -1.0, 0.33333334, 3.3895314e38]


def esize(dt: torch.dtype) -> int:
    return torch.empty((), dtype=dt).element_size()


def pairs():
    """Every (dtype, out) pair the schema accepts: out=None for each source, every float source to
    the four float outputs, every integer source to all six."""
    out = [(s, None) for s in SOURCES]
    for s in SOURCES:
        out += [(s, d) for d in OUTS if not (s.is_floating_point and d not in FLOATS)]
    return out


def layout(schema):
    """[(field, byte offset)] of a Struct."""
    return list(zip(schema.members, schema.offsets))


def float_values(dt: torch.dtype, n: int, g: torch.Generator) -> torch.Tensor:
    """n values of float dtype ``dt``: the specials (as far as ``dt`` holds them) first, then
    random finite values over many binades."""
    v = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 18, (n,), generator=g).float())
    k = min(n, len(SPECIALS_F32))
    v[:k] = torch.tensor(SPECIALS_F32[:k])
    return v.to(dt)


def random_records(schema, rows: int, seed: int = 0) -> torch.Tensor:
    """uint8 [rows, size]: random bytes everywhere (gaps and integer fields), float fields
    overwritten in declaration order with specials and random finite values."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (rows, schema.size), dtype=torch.uint8, generator=g)
    for f, off in layout(schema):
        if f.dtype.is_floating_point and rows:
            vals = float_values(f.dtype, rows * f.elems, g)
            vals = vals[torch.randperm(rows * f.elems, generator=g)]  # the specials land in every column
            raw[:, off:off + f.nbytes] = vals.view(rows, f.elems).view(torch.uint8)
    return raw


def _affine(f):
    if f.normalize is None:
        return None
    mean, std = (torch.as_tensor(t, dtype=torch.float32).flatten() for t in f.normalize)
    mean = mean.expand(f.elems) if mean.numel() == 1 else mean
    std = std.expand(f.elems) if std.numel() == 1 else std
    return mean, torch.tensor(1.0, dtype=torch.float32) / std


def oracle_field(f, chunk: bytearray) -> torch.Tensor:
    """One record's field from its own bytes -> a flat tensor of ``f.elems`` elements."""
    dest = f.dtype if f.out is None else f.out
    if f.out is None and f.normalize is None:
        return torch.frombuffer(chunk, dtype=f.dtype)
    x = torch.frombuffer(chunk, dtype=f.dtype)
    if dest not in FLOATS:
        return x.to(dest)
    y = x.to(torch.float32)
    aff = _affine(f)
    if aff is not None:
        y = (y - aff[0]) * aff[1]
    return y.to(dest)


def oracle(raw: torch.Tensor, schema) -> dict:
    """uint8 [rows, size] -> {name: tensor [rows, *shape]}, row by row and field by field."""
    rows = raw.shape[0]
    data = [bytes(r.tolist()) for r in raw]
    out = {}
    for f, off in layout(schema):
        dest = f.dtype if f.out is None else f.out
        got = [oracle_field(f, bytearray(row[off:off + f.nbytes])) for row in data]
        t = torch.stack(got) if rows else torch.empty((0, f.elems), dtype=dest)
        out[f.name] = t.view(rows, *f.shape)
    return out


def oracle_record(value: bytes, schema) -> dict:
    """One record value -> {name: tensor [*shape]}."""
    return {f.name: oracle_field(f, bytearray(value[off:off + f.nbytes])).view(f.shape) for f, off in layout(schema)}


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(_BITS[t.element_size()])


def assert_field_equal(f, got: torch.Tensor, want: torch.Tensor, what: str = "") -> None:
    dest = f.dtype if f.out is None else f.out
    assert got.dtype == want.dtype == dest, (what, f.name, got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), (what, f.name, tuple(got.shape), tuple(want.shape))
    gb, wb = bits(got), bits(want)
    if (f.out is None and f.normalize is None) or dest not in FLOATS:
        bad = gb != wb
    else:
        gf, wf = got.detach().cpu().to(torch.float32), want.to(torch.float32)
        assert torch.equal(gf.isnan(), wf.isnan()), (what, f.name, "NaN positions differ")
        bad = (gb != wb) & ~wf.isnan()
    if bool(bad.any()):
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(f"{what} field {f.name!r}: {int(bad.sum())} elements differ, first at flat index {i}: "
                             f"got bits {int(gb.flatten()[i]):#x}, want {int(wb.flatten()[i]):#x}")


def assert_struct_equal(schema, got: dict, want: dict, what: str = "") -> None:
    assert list(got) == [f.name for f in schema.members], (what, list(got))
    for f in schema.members:
        assert_field_equal(f, got[f.name], want[f.name], what)


def offsets52():
    """The 52-byte test record: rows start at every residue of 4 mod 16; the fields cover offset
    residues 0-3 mod 4, an i64 off its natural alignment, and a gap up to 52."""
    from torchkafka_amd import Field

    return (Field("u", U8), Field("f", F32, (3,)), Field("q", I64), Field("b", BF16, (5,)), Field("h", F16),
            Field("c", I8, (2,)), Field("i", I32, (2,)))


def struct52(**kw):
    from torchkafka_amd import Struct

    s = Struct(*offsets52(), size=52, **kw)
    assert s.offsets == (0, 1, 13, 21, 31, 33, 35) and s.size == 52
    return s


def all_pairs_struct(normalize: str | None):
    """One field of three elements per accepted (dtype, out) pair, packed at odd offsets; float
    destinations normalised with a scalar or a per-element mean / std."""
    from torchkafka_amd import Field, Struct

    g = torch.Generator().manual_seed(5)
    fields, structs = [], []
    for i, (src, out) in enumerate(pairs()):
        dest = src if out is None else out
        norm = None
        if normalize is not None and dest in FLOATS:
            norm = (0.375, 1.7) if normalize == "scalar" else (torch.randn(3, generator=g),
                                                               torch.rand(3, generator=g) + 0.5)
        fields.append(Field(f"p{i}", src, (3,), out=out, normalize=norm))
        if len(fields) == 22:  # 43 pairs: two structs of at most 32 fields
            structs.append(fields)
            fields = []
    structs.append(fields)
    out = []
    for fs in structs:
        fs = [Field("lead", U8)] + fs  # every field after it sits one byte off
        end = 1 + sum(f.nbytes for f in fs[1:])
        out.append(Struct(*fs, size=(end + 3) // 4 * 4))
    return out


def le(fmt: str, *vals) -> bytes:
    return pystruct.pack("<" + fmt, *vals)


# ----------------------------------------------------------------------------- loader tests
PARTS, PER_PART, BS = 3, 70, 32


def produce_struct(broker, schema, seed=0, bad_at=None):
    """PARTS x PER_PART records of ``schema`` with keys of 0-8 bytes (every value's alignment in the
    log shifts) -> the produced rows per partition, uint8 [PER_PART, size].  ``bad_at``: (partition,
    index) of one extra record of a wrong size.  The first element of field ``i`` of the 52-byte
    struct is overwritten with partition * 1000 + index."""
    import random

    rng = random.Random(seed)
    broker.create_topic("t", PARTS)
    rows = []
    for p in range(PARTS):
        raw = random_records(schema, PER_PART, seed * 100 + p)
        stamp = torch.arange(p * 1000, p * 1000 + PER_PART, dtype=torch.int32)  # i[:, 0]: which record a row is
        raw[:, 35:39] = stamp.view(-1, 1).view(torch.uint8)
        vals = [bytes(r.tolist()) for r in raw]
        if bad_at is not None and bad_at[0] == p:
            vals.insert(bad_at[1], b"\x01" * (schema.size - 4))
        keys = [b"k" * rng.randrange(0, 9) for _ in vals]
        broker.produce("t", vals, partition=p, keys=keys)
        rows.append(raw)
    return rows


def check_batches(schema, rows, batches, device_type, sizes=None):
    """The delivered dicts, concatenated and put into the produced order by the stamp in ``i[:, 0]``
    (batches interleave the partitions), equal the oracle over the produced bytes; every partition's
    records arrive in offset order."""
    want = oracle(torch.cat(rows), schema)
    for b in batches:
        assert isinstance(b, dict) and all(v.device.type == device_type for v in b.values())
    if sizes is not None:
        assert [next(iter(b.values())).shape[0] for b in batches] == sizes
    got = {f.name: torch.cat([b[f.name].cpu() for b in batches]) for f in schema.members}
    stamps = got["i"][:, 0]
    assert stamps.numel() == PARTS * PER_PART
    for p in range(PARTS):
        mine = stamps[(stamps >= p * 1000) & (stamps < p * 1000 + 1000)]
        assert mine.tolist() == list(range(p * 1000, p * 1000 + PER_PART)), f"partition {p} out of order"
    order = torch.argsort(stamps)
    got = {k: v[order] for k, v in got.items()}
    assert_struct_equal(schema, got, want, "loader")
