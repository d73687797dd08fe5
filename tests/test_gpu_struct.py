"""struct_split.hip at the kernel level, through the pointer binding ``hip().struct_split``: every
output is a view into a canary-filled buffer with guard rows before and behind it, the input sits
at a chosen residue of 4 mod 16, and the results are compared with the loop oracle of
``helpers/structs.py`` (bytes; converted floats by NaN positions, then bytes)."""
import pytest
import torch

from helpers import structs as S
from helpers.structs import BF16, F16, F32, I8, I32, I64, U8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 3  # guard rows on each side of every output


def _mod():
    from torchkafka_amd.ops.native import hip

    return hip()


def place_raw(raw: torch.Tensor, residue: int):
    """The records on the device, starting ``residue`` bytes behind a 16-byte boundary, inside a
    buffer with canary bytes around them (the kernel only reads it: the canaries show up in a field
    if it reads out of range)."""
    n = raw.numel()
    buf = torch.full((n + 64,), CANARY, dtype=U8, device=DEV)
    start = (-buf.data_ptr()) % 16 + residue
    buf[start:start + n] = raw.flatten().to(DEV)
    return buf, buf.data_ptr() + start


def guarded_outputs(schema, rows: int):
    """Per field a canary-filled buffer of rows + 2 * GUARD rows and the address of row GUARD."""
    bufs, ptrs = [], []
    for f in schema.members:
        per_row = f.elems * S.esize(f.out_dtype)
        b = torch.full(((rows + 2 * GUARD) * per_row,), CANARY, dtype=U8, device=DEV)
        bufs.append(b)
        ptrs.append(b.data_ptr() + GUARD * per_row)
    return bufs, ptrs


def table_of(schema, ptrs):
    return [(off, f.elems, src, dst, p, shift, scale)
            for (off, _shape, src, dst, shift, scale), f, p in zip(schema.device_spec(DEV), schema.members, ptrs)]


def read_outputs(schema, bufs, rows: int):
    """-> the field tensors; asserts that every guard row still holds the canary."""
    out = {}
    for f, b in zip(schema.members, bufs):
        per_row = f.elems * S.esize(f.out_dtype)
        host = b.cpu()
        lo, hi = GUARD * per_row, (GUARD + rows) * per_row
        assert bool((host[:lo] == CANARY).all()), f"field {f.name!r}: wrote before its first row"
        assert bool((host[hi:] == CANARY).all()), f"field {f.name!r}: wrote behind its last row"
        out[f.name] = host[lo:hi].clone().view(f.out_dtype).view(rows, *f.shape)
    return out


def run_kernel(schema, raw: torch.Tensor, residue: int = 0, stream=None):
    rows = raw.shape[0]
    keep, raw_ptr = place_raw(raw, residue)
    bufs, ptrs = guarded_outputs(schema, rows)
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    _mod().struct_split(raw_ptr, rows, schema.size, table_of(schema, ptrs), s.cuda_stream)
    s.synchronize()
    del keep
    return read_outputs(schema, bufs, rows)


def check(schema, rows: int, seed: int = 0, residue: int = 0, stream=None, what: str = ""):
    raw = S.random_records(schema, rows, seed)
    got = run_kernel(schema, raw, residue, stream)
    S.assert_struct_equal(schema, got, S.oracle(raw, schema), what or f"{rows} rows, residue {residue}")


# ----------------------------------------------------------------------------- offsets and row counts
def test_tile_rows_rule():
    """The row counts below are tile edges only if the tile is what this test says it is."""
    m = _mod()
    assert [m.struct_tile_rows(r, 52) for r in (1, 64, 257, 2016, 2017, 4032, 4033)] == [16, 16, 16, 16, 32, 32, 64]
    assert m.struct_tile_rows(3, 32768) == 1 and m.struct_tile_rows(70, 1204) == 27
    assert m.struct_tile_rows(200, 1024) == 16 and m.struct_tile_rows(10 ** 6, 1024) == 32


# 1, 63, 64, 65, 257: wave and 64-row tile edges; 15-17, 33: the edges of the 16-row tile a small batch
# gets; 2049: 32-row tiles with a one-row last tile; 4097: 64-row tiles (and a one-row last tile)
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 63, 64, 65, 257, 2049, 4097])
def test_field_offsets_at_every_row_count(rows):
    """The 52-byte record: with 13 dwords per row the tiles start at every residue of 4 mod 16 (on
    top of the residue the batch itself starts at); the fields sit at offset residues 0-3 mod 4,
    the i64 off its natural alignment."""
    check(S.struct52(), rows, seed=rows, residue=4 * (rows % 4))


@pytest.mark.parametrize("residue", [0, 4, 8, 12])
def test_every_start_residue(residue):
    check(S.struct52(), 70, seed=residue, residue=residue)


def test_wide_field():
    """f32[300] in a 1204-byte record: 27-row tiles, 8100 pairs of one field dealt over the waves."""
    from torchkafka_amd import Field, Struct

    s = Struct(Field("lead", U8), Field("wide", F32, (300,), out=BF16, normalize=(0.25, 3.0)), size=1204)
    assert s.offsets == (0, 1)
    check(s, 70, seed=1, residue=8)


def test_even_pitch_record_with_scalar_fields():
    """A 1024-byte record (256 dwords a row: the pitch the kernel pads) read at a stride of one row."""
    from torchkafka_amd import Field, Struct

    s = Struct(Field("a", I32, offset=512), Field("h", F16, out=F32, offset=3), Field("q", I64, out=I32, offset=1015),
               Field("last", U8, offset=1023), Field("first", I8, out=I64, offset=0), Field("v", F32, (7,), offset=101),
               size=1024)
    check(s, 200, seed=2, residue=4)


def test_largest_record():
    """32768 bytes, one row per tile; the last field ends with the record."""
    from torchkafka_amd import Field, Struct

    s = Struct(Field("first", U8), Field("mid", F32, (100,), out=F16, offset=16383),
               Field("odd", BF16, (3,), offset=32753), Field("last", I64, offset=32760),
               Field("all", I32, (8192,), offset=0), size=32768)
    check(s, 3, seed=3, residue=12)


def test_32_one_element_fields_and_an_overlap():
    from torchkafka_amd import Field, Struct

    dts = (U8, F32, I64, BF16, F16, I8, I32)
    s = Struct(*(Field(f"f{i}", dts[i % 7], out=(F32 if i % 3 == 0 else None)) for i in range(32)), size=112)
    assert len(s.members) == 32
    for rows in (5, 130):
        check(s, rows, seed=rows)
    u = Struct(Field("wide", I64, offset=2), Field("lo", I32, offset=2), Field("hi", I32, offset=6),
               Field("by", U8, (8,), out=I32, offset=2), Field("mid", F32, out=BF16, offset=4), size=12)
    raw = S.random_records(u, 90, 4)
    got = run_kernel(u, raw)
    S.assert_struct_equal(u, got, S.oracle(raw, u), "overlap")
    assert torch.equal((got["hi"].long() << 32) | (got["lo"].long() & 0xFFFFFFFF), got["wide"])


# ----------------------------------------------------------------------------- dtypes
@pytest.mark.parametrize("normalize", [None, "scalar", "vector"])
def test_every_dtype_pair(normalize):
    """Every (dtype, out) pair the schema accepts, three elements each, one byte off alignment."""
    seen = set()
    for s in S.all_pairs_struct(normalize):
        check(s, 80, seed=7, what=f"normalize={normalize}")
        seen |= {(f.dtype, f.out) for f in s.members[1:]}
    assert seen == set(S.pairs()) and len(seen) == 43


# ----------------------------------------------------------------------------- streams, empty input, the op
def test_non_default_stream():
    side = torch.cuda.Stream(DEV)
    check(S.struct52(), 100, seed=5, residue=4, stream=side)


def test_no_rows_no_launch():
    from torchkafka_amd import split_struct

    s = S.struct52()
    bufs, ptrs = guarded_outputs(s, 0)
    _mod().struct_split(0, 0, s.size, table_of(s, ptrs), 0)  # a null input is fine: nothing is launched
    _mod().struct_split(0, 0, s.size, table_of(s, [0] * len(ptrs)), 0)
    torch.cuda.synchronize()
    read_outputs(s, bufs, 0)
    got = split_struct(torch.empty((0, 13), dtype=I32, device=DEV), s)
    assert {k: (v.dtype, tuple(v.shape), v.device.type) for k, v in got.items()} == {
        f.name: (f.out_dtype, (0, *f.shape), "cuda") for f in s.members}


def test_split_struct_op_on_device_tensors():
    """The tensor-level entry: int32 carrier and uint8 rows, a view that starts off a dword, and a
    side stream as the current one; equal to ``reference_struct`` on the same device too."""
    from torchkafka_amd import reference_struct, split_struct

    for s in S.all_pairs_struct("vector") + [S.struct52()]:
        raw = S.random_records(s, 77, 8)
        want = S.oracle(raw, s)
        dev = raw.to(DEV)
        S.assert_struct_equal(s, split_struct(dev, s), want, "uint8")
        S.assert_struct_equal(s, split_struct(dev.view(I32), s), want, "int32")
        S.assert_struct_equal(s, reference_struct(dev, s), want, "reference_struct on the device")
        odd = torch.empty(raw.numel() + 1, dtype=U8, device=DEV)[1:].view(77, s.size)
        odd.copy_(dev)
        assert odd.data_ptr() % 4 == 1
        S.assert_struct_equal(s, split_struct(odd, s), want, "view off a dword")
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            got = split_struct(dev, s)
        side.synchronize()
        S.assert_struct_equal(s, got, want, "side stream")


# ----------------------------------------------------------------------------- launcher refusals
def test_launcher_refusals_write_nothing():
    m = _mod()
    s = S.struct52()
    rows = 8
    raw = S.random_records(s, rows, 6)
    keep, raw_ptr = place_raw(raw, 0)
    bufs, ptrs = guarded_outputs(s, rows)
    good = table_of(s, ptrs)
    f32, i32, i64, copy = 0, 6, 7, int(m.STRUCT_COPY)
    norm = torch.ones(4, device=DEV)

    def entry(k, **kw):
        names = ("src_off", "elems", "src_dt", "dst_dt", "dst", "shift", "scale")
        e = dict(zip(names, good[k]))
        e.update(kw)
        return tuple(e[n] for n in names)

    def swapped(k, **kw):
        return good[:k] + [entry(k, **kw)] + good[k + 1:]

    bad = [
        ("fields", (raw_ptr, rows, 52, good * 5)),                                   # 35 fields
        ("fields", (raw_ptr, rows, 52, [])),
        ("inside the record", (raw_ptr, rows, 52, swapped(6, src_off=45))),          # i32[2] at 45 ends at 53
        ("inside the record", (raw_ptr, rows, 52, swapped(2, src_off=-1))),
        ("inside the record", (raw_ptr, rows, 52, swapped(2, elems=0))),
        ("inside the record", (raw_ptr, rows, 40, good)),                            # the record shrank under them
        ("multiple of 4", (raw_ptr, rows, 54, good)),
        ("multiple of 4", (raw_ptr, rows, 32772, good)),
        ("null output", (raw_ptr, rows, 52, swapped(3, dst=0))),
        ("null input", (0, rows, 52, good)),
        ("4-byte aligned", (raw_ptr + 2, rows, 52, good)),
        ("aligned to its element size", (raw_ptr, rows, 52, swapped(2, dst=ptrs[2] + 4))),
        (r"2\^31", (raw_ptr, (1 << 31) // 52 + 1, 52, good)),
        (r"2\^31", (raw_ptr, -1, 52, good)),
        ("unsupported source", (raw_ptr, rows, 52, swapped(0, src_dt=3))),           # fp8 is no source
        ("unsupported source", (raw_ptr, rows, 52, swapped(0, src_dt=8))),
        ("unsupported destination", (raw_ptr, rows, 52, swapped(0, dst_dt=4))),      # uint8 is no conversion target
        ("unsupported destination", (raw_ptr, rows, 52, swapped(0, dst_dt=-2))),
        ("no integer destination", (raw_ptr, rows, 52, swapped(1, dst_dt=i32))),     # f32 -> int32
        ("no integer destination", (raw_ptr, rows, 52, swapped(4, dst_dt=i64))),     # f16 -> int64
        ("come together", (raw_ptr, rows, 52, swapped(1, dst_dt=f32, shift=norm.data_ptr()))),
        ("float destination", (raw_ptr, rows, 52, swapped(6, dst_dt=i64, shift=norm.data_ptr(),
                                                         scale=norm.data_ptr()))),
        ("float destination", (raw_ptr, rows, 52, swapped(1, dst_dt=copy, shift=norm.data_ptr(),
                                                         scale=norm.data_ptr()))),
    ]
    for msg, args in bad:
        with pytest.raises(ValueError, match=msg):
            m.struct_split(*args, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    for f, b in zip(s.members, bufs):
        assert bool((b.cpu() == CANARY).all()), f"a refused launch wrote to field {f.name!r}"
    # and the table they were all derived from is good
    m.struct_split(raw_ptr, rows, 52, good, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    S.assert_struct_equal(s, read_outputs(s, bufs, rows), S.oracle(raw, s), "the good table")
    del keep
