"""The MX block-scaled formats without a GPU: ``reference_mx`` against the scalar oracle
(tests/helpers/mx.py) byte for byte, ``MXBatch.dequantize``, the argument and configuration refusals,
and ``DeviceLoader(device="cpu", quantize=...)`` against ``reference_mx`` of the batch a second loader
over the same topic delivers without ``quantize``."""
import struct

import pytest
import torch

from helpers import mx
from helpers.known_records import known_rows, row_bytes
from test_gpu_loader_reference import _dataset, _loader

F32, BF16, F16, FP8 = torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn
CASES = [(d, f) for d in mx.DTYPES for f in mx.FORMATS]


# ----------------------------------------------------------------------------- the op
def test_the_table_holds_the_cases_it_names():
    blocks, notes = mx.mx_blocks(), mx.block_notes()
    assert blocks.shape == (len(notes), 32)
    finite = torch.isfinite(blocks).all(dim=1)
    amax = blocks.abs().max(dim=1).values
    for what in ("one NaN", "one +Inf", "one -Inf"):
        assert not finite[[i for i, n in enumerate(notes) if n.startswith(what)]].any()
    assert bool((amax[finite] == 0).any()) and bool(((amax > 0) & (amax < 2.0 ** -126)).any())  # zero, subnormal
    assert bool((amax == mx.FLT_MAX).any())
    neg0 = blocks[notes.index("all -0.0 #0")].view(torch.int32)
    assert bool((neg0 == -0x80000000).all())
    at256 = blocks[[i for i, n in enumerate(notes) if n.startswith("anchored at 256")]]
    assert bool(((at256.abs().max(dim=1).values >= 256) & (at256.abs().max(dim=1).values < 512)).all())
    assert bool((at256.abs() > 448).any()) and bool((at256 == 464.0).any())
    at4 = blocks[[i for i, n in enumerate(notes) if n.startswith("anchored at 4")]]
    assert bool(((at4.abs().max(dim=1).values >= 4) & (at4.abs().max(dim=1).values < 8)).all())
    for m in mx.E2M1_MIDPOINTS:
        assert bool((at4 == m).any()) and bool((at4 == -m).any())


def test_the_oracle_on_hand_worked_blocks():
    """Blocks worked by hand from the rules, so the oracle itself is pinned."""
    blk = [0.0] * 32
    assert mx.oracle_block(blk, "mxfp8") == (0, [0] * 32)                   # E = -127 clamps to se = -127
    blk[3], blk[4], blk[5], blk[6] = 256.0, -464.0, 500.0, -0.0             # se = 0: clamp, then the e4m3fn cast
    s, v = mx.oracle_block(blk, "mxfp8")
    assert s == 127 and v[3] == 0x78 and v[4] == 0xFE and v[5] == 0x7E and v[6] == 0x80 and v[0] == 0
    blk = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -5.0, 7.5, -0.0, 0.26, 0.74] + [0.0] * 18
    s, v = mx.oracle_block(blk, "mxfp4")
    codes = [c for byte in v for c in (byte & 0xF, byte >> 4)]
    assert s == 127 and codes[:14] == [6, 0, 2, 2, 4, 4, 6, 6, 8, 14, 7, 8, 1, 1]
    assert mx.oracle_block([float("inf")] + [1.0] * 31, "mxfp4") == (0xFF, [0] * 16)
    assert mx.oracle_block([1.0] * 32, "mxfp8")[0] == 127 - 8 and mx.oracle_block([1.0] * 32, "mxfp4")[0] == 127 - 2
    assert mx.oracle_block([2.0 ** -140] * 32, "mxfp8")[0] == 0
    assert mx.oracle_block([mx.FLT_MAX] * 32, "mxfp8") == (127 + 127 - 8, [0x7E] * 32)  # 511.99.. saturates to 448


@pytest.mark.parametrize("dt,fmt", CASES)
def test_reference_mx_matches_the_oracle(dt, fmt):
    from torchkafka_amd import reference_mx

    x = mx.table(mx.DTYPES[dt])
    want_v, want_s = mx.oracle_table(mx.DTYPES[dt], fmt)
    got = reference_mx(x, fmt)
    assert got.fmt == fmt and got.scales.dtype == torch.uint8 and tuple(got.scales.shape) == (x.shape[0], 1)
    if fmt == "mxfp8":
        assert got.values.dtype == FP8 and got.values.shape == x.shape
    else:
        assert got.values.dtype == torch.uint8 and tuple(got.values.shape) == (x.shape[0], 16)
    mx.assert_mx_equal(got, want_v, want_s, f"{dt} {fmt}")


@pytest.mark.parametrize("fmt", mx.FORMATS)
def test_shapes_views_and_non_contiguous_inputs(fmt):
    from torchkafka_amd import MXBatch, quantize_mx, reference_mx

    x, want_v, want_s = mx.pick(range(40, 52), F32, fmt)
    got = quantize_mx(x.reshape(3, 2, 64), fmt)  # a CPU tensor: the reference
    assert isinstance(got, MXBatch) and tuple(got.scales.shape) == (3, 2, 2)
    assert tuple(got.values.shape) == ((3, 2, 64) if fmt == "mxfp8" else (3, 2, 32))
    mx.assert_mx_equal(got, want_v, want_s, "rank 3")
    t = x.reshape(6, 64).t().contiguous().t()  # [6, 64] with strides (1, 6)
    assert not t.is_contiguous()
    mx.assert_mx_equal(reference_mx(t, fmt), want_v, want_s, "transposed")
    assert got.scales_e8m0.dtype == torch.float8_e8m0fnu and got.scales_e8m0.shape == got.scales.shape
    if fmt == "mxfp4":
        assert got.values_fp4x2.dtype == torch.float4_e2m1fn_x2 and got.values_fp4x2.shape == got.values.shape
    else:
        with pytest.raises(TypeError):
            _ = got.values_fp4x2
    empty = reference_mx(torch.zeros(0, 64), fmt)
    assert tuple(empty.scales.shape) == (0, 2) and empty.values.shape[0] == 0


@pytest.mark.parametrize("dt,fmt", CASES)
def test_dequantize_round_trips(dt, fmt):
    """|deq - x| <= amax_block * 2^-3 (mxfp8) / 2^-1 (mxfp4) on every block with a finite scale that
    did not clamp; measured 0.125 / 0.25 of amax at most, the saturation of the top binade.  A block
    whose scale exponent clamped at -127 (amax below 2^(emax - 126)) cannot meet a bound relative to
    amax -- its elements fall below the format's smallest step -- so there the bound is half that
    step, 2^-127 * 2^-10 (e4m3fn's smallest subnormal is 2^-9) / 2^-127 * 2^-2 (e2m1's is 0.5).  A
    bad block dequantises to NaN everywhere."""
    from torchkafka_amd import reference_mx

    emax, _top = mx.EMAX_TOP[fmt]
    x = mx.table(mx.DTYPES[dt])
    q = reference_mx(x, fmt)
    deq = q.dequantize()
    assert deq.dtype == F32 and deq.shape == x.shape
    xf = x.to(torch.float64)
    s = q.scales.reshape(-1)
    bad = s == 255
    assert bool(torch.isnan(deq[bad]).all()) and bool(torch.isfinite(deq[~bad]).all())
    assert torch.equal(bad, ~torch.isfinite(xf).all(dim=1))
    amax = xf.abs().max(dim=1).values
    rel = 2.0 ** -3 if fmt == "mxfp8" else 2.0 ** -1
    half_step = 2.0 ** -127 * (2.0 ** -10 if fmt == "mxfp8" else 2.0 ** -2)
    clamped = s == 0
    assert bool((amax[clamped] < 2.0 ** (emax - 126)).all())
    assert bool((amax[~clamped & ~bad] >= 2.0 ** (emax - 127)).all())
    bound = torch.where(clamped, torch.maximum(amax * rel, torch.full_like(amax, half_step)), amax * rel)
    err = (deq.to(torch.float64) - xf).abs()
    ok = ~bad
    worst = (err[ok] / amax[ok].clamp(min=1e-300)[:, None])[~clamped[ok]].max()
    print(f"{dt} {fmt}: worst |deq - x| / amax over unclamped blocks = {float(worst):.4f}")
    assert bool((err[ok] <= bound[ok][:, None]).all())
    assert q.dequantize(BF16).dtype == BF16
    # an exactly representable block comes back exactly
    exact = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0] * 4) * 2.0 ** -20
    exact[1::2] = -exact[1::2]
    assert torch.equal(reference_mx(exact.to(mx.DTYPES[dt]), fmt).dequantize(), exact)


def test_argument_errors():
    from torchkafka_amd import quantize_mx, reference_mx

    for fn in (quantize_mx, reference_mx):
        with pytest.raises(ValueError, match="multiple of 32"):
            fn(torch.zeros(4, 48), "mxfp8")
        with pytest.raises(ValueError, match="multiple of 32"):
            fn(torch.zeros(()), "mxfp8")
        with pytest.raises(ValueError, match="fmt"):
            fn(torch.zeros(4, 64), "mxfp6")
        for dt in (torch.int32, torch.float64, FP8, torch.uint8):
            with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
                fn(torch.zeros(4, 64).to(dt), "mxfp4")
    assert quantize_mx(torch.zeros(2, 32)).fmt == "mxfp8"  # the default format


# ----------------------------------------------------------------------------- configuration
@pytest.mark.parametrize("opts,msg", [
    ({"quantize": "fp8"}, "quantize"),
    ({"quantize": "mxfp6"}, "quantize"),
    ({"quantize": "mxfp8", "layout": "packed"}, "quantize needs layout='padded'"),
    ({"quantize": "mxfp4", "layout": "binned", "seq_len": 64}, "quantize needs layout='padded'"),
])
def test_config_refuses(opts, msg):
    from torchkafka_amd import LoaderConfig

    with pytest.raises(ValueError, match=msg):
        LoaderConfig(**opts)
    with pytest.raises(ValueError, match=msg):
        LoaderConfig.build(None, **opts)


def test_config_accepts_quantize():
    from torchkafka_amd import LoaderConfig

    assert LoaderConfig().quantize is None
    for q in ("mxfp8", "mxfp4"):
        cfg = LoaderConfig.build(None, quantize=q)
        assert cfg.quantize == q and LoaderConfig.from_dict(cfg.to_dict()).quantize == q


def _construct(schema, **kw):
    from torchkafka_amd import DeviceLoader

    DS = _dataset(schema)
    return DeviceLoader(DS.placeholder(), 4, num_workers=1, device="cpu",
                        worker_init_fn=DS.init_worker("t", bootstrap_servers="shm://nowhere", group_id="g"), **kw)


def test_construction_time_refusals():
    from torchkafka_amd import FixedWidth, JsonArray, Key, VarLen

    fixed, var = FixedWidth(F32, (64,)), VarLen(F32)
    narrow = FixedWidth(F32, (48,))
    for schema in (narrow, FixedWidth(F32, (32, 8)), FixedWidth(F32, ()), narrow + Key()):
        with pytest.raises(ValueError, match="multiple of 32"):
            _construct(schema, quantize="mxfp8")
    # (pad_multiple defaults to 8)
    for kw in ({}, {"pad_multiple": 16}, {"pad_to": 48}, {"pad_to": 48, "pad_multiple": 32}):
        for schema in (var, JsonArray()):
            with pytest.raises(ValueError, match="multiple of 32"):
                _construct(schema, quantize="mxfp4", **kw)
    for schema, kw in ((FixedWidth(torch.int32, (64,)), {}), (FixedWidth(torch.uint8, (64,)), {}),
                       (fixed, {"dtype": FP8}), (fixed, {"dtype": torch.int32}),
                       (VarLen(torch.int64), {"pad_multiple": 32}), (var, {"pad_multiple": 32, "dtype": FP8}),
                       (JsonArray(), {"pad_to": 64, "dtype": FP8})):
        with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
            _construct(schema, quantize="mxfp8", **kw)
    with pytest.raises(TypeError, match="structured"):
        _construct(None, quantize="mxfp8")
    for kw in ({"layout": "packed"}, {"layout": "binned", "seq_len": 64}):
        with pytest.raises(ValueError, match="layout='padded'"):
            _construct(var, quantize="mxfp8", pad_multiple=32, **kw)
    # what is accepted
    for schema, kw in ((fixed, {}), (FixedWidth(F32, (4, 32)), {"dtype": BF16}), (fixed + Key(), {"dtype": F16}),
                       (FixedWidth(torch.int32, (64,)), {"dtype": F32}), (var, {"pad_multiple": 32}),
                       (var, {"pad_to": 64}), (JsonArray(), {"pad_multiple": 64, "dtype": BF16})):
        for q in mx.FORMATS:
            assert _construct(schema, quantize=q, **kw).quantize == q
    assert _construct(fixed).quantize is None


# ----------------------------------------------------------------------------- the loader
N, RPB, BS = 103, 7, 32


def fixed_rows(width: int = 64):
    """N known f32 rows (specials, ties, NaN and Inf included) as record values."""
    return [row_bytes(r) for r in known_rows(F32, (width,), N, 311)]


def varlen_rows():
    """N var-len f32 rows of 0..70 elements (so the batch width is 32, 64 or 96 with pad_multiple=32)."""
    g = torch.Generator().manual_seed(17)
    lens = torch.randint(0, 71, (N,), generator=g).tolist()
    for i in range(2 * BS, 3 * BS):  # one batch of short rows: its width is 32
        lens[i] %= 30
    lens[0], lens[1], lens[20], lens[40] = 0, 32, 70, 33  # the first batch is 96 wide
    vals = known_rows(F32, (1,), sum(lens), 313).flatten()
    out, pos = [], 0
    for k in lens:
        out.append(row_bytes(vals[pos:pos + k]))
        pos += k
    return out


def keys_be():
    return [struct.pack(">q", 5000 + 3 * i) for i in range(N)]


def paired_run(broker, schema, device, fmt, values, keys=None, **kw):
    """The records into one partition; then the same loader twice, under two group ids: without
    ``quantize`` and with it.  -> (the quantising loader, plain batches, quantised batches)."""
    from torchkafka_amd import auto_commit

    broker.create_topic("t", 1)
    for i in range(0, len(values), RPB):
        broker.produce("t", values[i:i + RPB], partition=0, keys=None if keys is None else keys[i:i + RPB])
    DS = _dataset(schema)
    plain = list(auto_commit(_loader(broker, DS, BS, device, "plain", **kw)))
    dl = _loader(broker, DS, BS, device, "mx", quantize=fmt, **kw)
    quant = list(auto_commit(dl))
    return dl, plain, quant


def parts(item):
    """A delivered item -> (the values tensor or MXBatch, the tensors riding with it)."""
    from torchkafka_amd import KafkaBatch, MXBatch

    if isinstance(item, KafkaBatch):
        return item.data, tuple(t for t in (item.lengths, item.mask) if t is not None)
    if isinstance(item, (MXBatch, torch.Tensor)):
        return item, ()
    return item[0], tuple(item[1:])


def check_pair(plain, quant, fmt, device_type, n_batches, n_riders):
    """Every quantised batch is reference_mx (on the CPU) of the plain batch, byte for byte; whatever
    rides with the values (lengths, mask, key) is equal."""
    from torchkafka_amd import MXBatch, reference_mx

    assert len(plain) == len(quant) == n_batches
    for b, (p, q) in enumerate(zip(plain, quant)):
        (pv, pr), (qv, qr) = parts(p), parts(q)
        assert isinstance(pv, torch.Tensor) and isinstance(qv, MXBatch) and qv.fmt == fmt
        assert pv.device.type == qv.values.device.type == qv.scales.device.type == device_type
        want = reference_mx(pv.cpu(), fmt)
        assert qv.values.dtype == want.values.dtype and qv.values.shape == want.values.shape
        assert qv.scales.shape == want.scales.shape
        mx.assert_mx_equal(qv, want.values.view(torch.uint8), want.scales, f"batch {b}")
        assert len(pr) == len(qr) == n_riders
        for a, c in zip(pr, qr):
            assert a.dtype == c.dtype and a.device.type == device_type and torch.equal(a.cpu(), c.cpu()), f"batch {b}"


@pytest.mark.parametrize("fmt", mx.FORMATS)
@pytest.mark.parametrize("case", ["fixed", "fixed+key", "varlen"])
def test_cpu_loader_delivers_reference_mx_of_the_plain_batch(broker, case, fmt):
    from torchkafka_amd import FixedWidth, Key, VarLen

    if case == "varlen":
        dl, plain, quant = paired_run(broker, VarLen(F32), "cpu", fmt, varlen_rows(), pad_multiple=32, pad_value=-1)
        assert {32, 96} <= {p[0].shape[1] for p in plain}
    else:
        schema = FixedWidth(F32, (64,)) + Key() if case == "fixed+key" else FixedWidth(F32, (64,))
        dl, plain, quant = paired_run(broker, schema, "cpu", fmt, fixed_rows(), keys_be())
    assert broker.committed_offsets("plain", "t") == broker.committed_offsets("mx", "t") == {0: N}
    check_pair(plain, quant, fmt, "cpu", (N + BS - 1) // BS, {"fixed": 0, "fixed+key": 1, "varlen": 1}[case])
    if case == "fixed+key":
        assert torch.cat([q[1] for q in quant]).tolist() == [5000 + 3 * i for i in range(N)]
