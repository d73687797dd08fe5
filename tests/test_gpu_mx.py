"""The MX quantise kernel (csrc/hip/mx_quant.hip) and ``DeviceLoader(quantize=...)`` on the GPU.

The kernel against the scalar oracle (tests/helpers/mx.py) and against ``reference_mx`` on the CPU, byte
for byte, on the table of input blocks: zero / -0.0 / NaN / Inf blocks, amax at and one ulp below powers
of two from 2^-149 to 2^127, FLT_MAX, the e4m3fn ties and the 448..512 range in blocks whose scale is 1,
every e2m1 midpoint with its neighbours, magnitudes from 2^-140 to 2^127.  The loader against
``reference_mx`` of the batch a second loader over the same topic delivers without ``quantize``."""
import json
import random

import pytest
import torch

from helpers import mx
from helpers.known_records import norm_vectors
from test_mx_cpu import BS, N, check_pair, fixed_rows, keys_be, paired_run, parts, varlen_rows

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CASES = [(d, f) for d in mx.DTYPES for f in mx.FORMATS]
DEV = "cuda:0"
# a partial lane group, a partial wave and a wave boundary for both lane-group sizes (8 lanes per block
# for f32 -> mxfp8: 8 blocks per wave; 4 lanes otherwise: 16 blocks per wave), and the whole table
COUNTS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def scattered(n: int) -> torch.Tensor:
    """``n`` block indices spread over the table, different for every ``n``."""
    total = mx.mx_blocks().shape[0]
    return (torch.arange(n) * 37 + 11 * n) % total


def check(x_cpu: torch.Tensor, got, want_v, want_s, fmt, what):
    """The kernel's batch against the oracle's bytes and against reference_mx of the same CPU tensor."""
    from torchkafka_amd import reference_mx

    assert got.fmt == fmt and got.values.is_cuda and got.scales.is_cuda
    ref = reference_mx(x_cpu, fmt)
    assert got.values.dtype == ref.values.dtype and got.values.shape == ref.values.shape
    assert got.scales.dtype == torch.uint8 and got.scales.shape == ref.scales.shape
    mx.assert_mx_equal(got, want_v, want_s, what + " vs the oracle")
    mx.assert_mx_equal(got, ref.values.view(torch.uint8), ref.scales, what + " vs reference_mx")


@pytest.mark.parametrize("dt,fmt", CASES)
def test_kernel_matches_the_oracle_at_every_block_count(dt, fmt):
    from torchkafka_amd import quantize_mx

    total = mx.mx_blocks().shape[0]
    for n in COUNTS + (total,):
        idx = torch.arange(total) if n == total else scattered(n)
        x, want_v, want_s = mx.pick(idx, mx.DTYPES[dt], fmt)
        flat = x.reshape(-1)  # 1-D: K = 32 n
        check(flat, quantize_mx(flat.to(DEV), fmt), want_v, want_s, fmt, f"{dt} {fmt} {n} blocks")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,fmt", CASES)
def test_kernel_grid_stride_loop(dt, fmt):
    """More blocks than the launch has lane groups: MX_MAX_GRID workgroups of 64 lane groups (32 for
    f32 -> mxfp8) take 131072 blocks a pass, so 131072 + 65 blocks send every instantiation through the
    loop again, the last pass with a partial wave."""
    from torchkafka_amd import quantize_mx
    from torchkafka_amd.ops.native import hip

    n = int(hip().MX_MAX_GRID) * 64 + 65
    idx = torch.arange(n) % mx.mx_blocks().shape[0]
    x, want_v, want_s = mx.pick(idx, mx.DTYPES[dt], fmt)
    got = quantize_mx(x.to(DEV), fmt)
    assert tuple(got.scales.shape) == (n, 1)
    mx.assert_mx_equal(got, want_v, want_s, f"{dt} {fmt} {n} blocks")


@pytest.mark.parametrize("dt,fmt", CASES)
def test_rank3_misaligned_transposed_and_side_stream(dt, fmt):
    from torchkafka_amd import quantize_mx

    dtype = mx.DTYPES[dt]
    x, want_v, want_s = mx.pick(scattered(12), dtype, fmt)
    # rank 3
    got = quantize_mx(x.reshape(3, 2, 64).to(DEV), fmt)
    assert tuple(got.scales.shape) == (3, 2, 2) and tuple(got.values.shape) == (3, 2, 64 if fmt == "mxfp8" else 32)
    check(x.reshape(3, 2, 64), got, want_v, want_s, fmt, "rank 3")
    # a view that starts 4 bytes past a 16-byte boundary
    off = 4 // x.element_size()
    base = torch.zeros(x.numel() + 16, dtype=dtype, device=DEV)
    base[off:off + x.numel()] = x.reshape(-1).to(DEV)
    view = base[off:off + x.numel()].view(6, 64)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    check(x.reshape(6, 64), quantize_mx(view, fmt), want_v, want_s, fmt, "misaligned view")
    # transposed: [6, 64] with strides (1, 6)
    t = x.reshape(6, 64).to(DEV).t().contiguous().t()
    assert not t.is_contiguous()
    check(x.reshape(6, 64), quantize_mx(t, fmt), want_v, want_s, fmt, "transposed")
    # on a side stream, read after its synchronize
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xs = x.to(DEV, non_blocking=True)
        got = quantize_mx(xs, fmt)
    s.synchronize()
    check(x, got, want_v, want_s, fmt, "side stream")
    # dequantize runs on the GPU and agrees with the CPU
    from torchkafka_amd import reference_mx

    a, b = got.dequantize().cpu(), reference_mx(x, fmt).dequantize()
    assert got.dequantize().is_cuda and torch.equal(torch.isnan(a), torch.isnan(b))
    normal = (b.abs() >= 2.0 ** -126) | (b == 0)  # a subnormal result may be flushed by the device's multiply
    assert torch.equal(a[normal], b[normal]) and bool(((a - b)[~normal & ~torch.isnan(b)].abs() < 2.0 ** -126).all())


def test_argument_errors_come_before_any_launch():
    from torchkafka_amd import quantize_mx
    from torchkafka_amd.ops.native import hip

    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_mx(torch.zeros(4, 48, device=DEV))
    with pytest.raises(ValueError, match="fmt"):
        quantize_mx(torch.zeros(4, 64, device=DEV), "mxfp6")
    with pytest.raises(TypeError):
        quantize_mx(torch.zeros(4, 64, device=DEV, dtype=torch.int32))
    # the native entries refuse what the kernel cannot take: a misaligned or non-contiguous source
    base = torch.zeros(4 * 64 + 4, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        hip().mx_tensors(base[1:1 + 4 * 64].view(4, 64), 0)
    with pytest.raises(ValueError, match="contiguous"):
        hip().mx_tensors(torch.zeros(64, 4, device=DEV).t(), 0)
    values, scales = torch.zeros(256, dtype=torch.uint8, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        hip().mx_quantize(base.data_ptr() + 4, 0, 8, 0, values.data_ptr(), scales.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip().mx_quantize(base.data_ptr(), 0, 8, 2, values.data_ptr(), scales.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip().mx_quantize(base.data_ptr(), 6, 8, 0, values.data_ptr(), scales.data_ptr(), 0)  # int32 source
    empty = quantize_mx(torch.zeros(0, 64, device=DEV), "mxfp4")
    assert tuple(empty.values.shape) == (0, 32) and tuple(empty.scales.shape) == (0, 2)
    torch.cuda.synchronize()
    assert not bool(values.any()) and not bool(scales.any())


def test_raw_binding_writes_the_same_bytes():
    from torchkafka_amd.ops.native import hip

    x, want_v, want_s = mx.pick(scattered(65), BF16, "mxfp4")
    xd = x.to(DEV)
    values = torch.empty(65 * 16, dtype=torch.uint8, device=DEV)
    scales = torch.empty(65, dtype=torch.uint8, device=DEV)
    hip().mx_quantize(xd.data_ptr(), 2, 65, 1, values.data_ptr(), scales.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(values.cpu(), want_v.reshape(-1)) and torch.equal(scales.cpu(), want_s)


# ----------------------------------------------------------------------------- the loader
W = 256
N_BATCHES = (N + BS - 1) // BS


def _on_gpu_and_committed(broker, quant):
    assert broker.committed_offsets("plain", "t") == broker.committed_offsets("mx", "t") == {0: N}
    for item in quant:
        q, riders = parts(item)
        assert q.values.is_cuda and q.scales.is_cuda and all(t.is_cuda for t in riders)


@pytest.mark.parametrize("path,opts,fmt", [
    ("span", dict(decode="device"), "mxfp8"),
    ("span", dict(decode="device"), "mxfp4"),
    ("host", dict(decode="host"), "mxfp4"),
    ("mirror", dict(decode="device", h2d="dma"), "mxfp8"),
    ("staged", dict(decode="host", h2d="dma"), "mxfp8"),
])
def test_fixed_width_loader_paths(broker, path, opts, fmt):
    from torchkafka_amd import FixedWidth

    dl, plain, quant = paired_run(broker, FixedWidth(F32, (W,)), DEV, fmt, fixed_rows(W), coalesce=4, **opts)
    assert dl.plan.fast_path and dl.plan.span == (path in ("span", "mirror")) and dl.plan.mirror == (path == "mirror")
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N_BATCHES, 0)
    assert all(tuple(q.values.shape) == (min(BS, N - BS * b), W if fmt == "mxfp8" else W // 2) and
               tuple(q.scales.shape) == (min(BS, N - BS * b), W // 32) for b, q in enumerate(quant))


@pytest.mark.parametrize("fmt", mx.FORMATS)
def test_fixed_width_with_a_key(broker, fmt):
    from torchkafka_amd import FixedWidth, Key

    dl, plain, quant = paired_run(broker, FixedWidth(F32, (W,)) + Key(), DEV, fmt, fixed_rows(W), keys_be(),
                                  decode="device", coalesce=4)
    assert dl.plan.fast_path and dl.plan.span
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N_BATCHES, 1)
    assert torch.cat([q[1] for q in quant]).tolist() == [5000 + 3 * i for i in range(N)]


@pytest.mark.parametrize("fmt", mx.FORMATS)
def test_bf16_with_normalize(broker, fmt):
    """The plain batch is the reference, so the normalise rounding is not in question."""
    from torchkafka_amd import FixedWidth

    mean, std = norm_vectors(W, 5)
    dl, plain, quant = paired_run(broker, FixedWidth(F32, (W,)), DEV, fmt, fixed_rows(W), decode="device", coalesce=4,
                                  dtype=BF16, normalize=(mean, std))
    assert all(p.dtype == BF16 for p in plain)
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N_BATCHES, 0)


@pytest.mark.parametrize("decode,fmt", [("device", "mxfp8"), ("host", "mxfp4")])
def test_varlen_with_mask(broker, decode, fmt):
    from torchkafka_amd import VarLen

    dl, plain, quant = paired_run(broker, VarLen(F32), DEV, fmt, varlen_rows(), decode=decode, coalesce=4,
                                  pad_multiple=32, pad_value=-1, return_mask=True)
    assert dl.plan.varlen_fast and dl.plan.var_span == (decode == "device")
    assert {32, 96} <= {p[0].shape[1] for p in plain}
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N_BATCHES, 2)
    assert all(len(q) == 3 and q[2].dtype == torch.bool for q in quant)


@pytest.mark.parametrize("fmt", mx.FORMATS)
def test_json_device_parse(broker, fmt):
    from torchkafka_amd import JsonArray

    rng = random.Random(41)
    texts = []
    for _ in range(N):
        vals = [round(rng.uniform(-1e4, 1e4), rng.randint(0, 6)) for _ in range(rng.randint(0, 70))]
        texts.append(("[" + ", ".join(repr(v) for v in vals) + "]").encode())
    dl, plain, quant = paired_run(broker, JsonArray(), DEV, fmt, texts, json_parse="device", coalesce=4,
                                  pad_multiple=32)
    assert dl.plan.json_device and dl.plan.varlen_fast
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N_BATCHES, 1)
    want = torch.tensor([len(json.loads(t)) for t in texts])
    assert torch.equal(torch.cat([q[1].cpu() for q in quant]), want)


@pytest.mark.parametrize("case,fmt", [("fixed", "mxfp4"), ("varlen", "mxfp8")])
def test_return_info_with_drop_last(broker, case, fmt):
    from torchkafka_amd import FixedWidth, KafkaBatch, MXBatch, VarLen

    if case == "fixed":
        dl, plain, quant = paired_run(broker, FixedWidth(F32, (W,)), DEV, fmt, fixed_rows(W), coalesce=4,
                                      return_info=True, drop_last=True)
    else:
        dl, plain, quant = paired_run(broker, VarLen(F32), DEV, fmt, varlen_rows(), coalesce=4, pad_multiple=32,
                                      return_info=True, drop_last=True)
    assert all(isinstance(q, KafkaBatch) and isinstance(q.data, MXBatch) for q in quant)
    assert [(q.n_records, q.watermarks) for q in quant] == [(p.n_records, p.watermarks) for p in plain]
    _on_gpu_and_committed(broker, quant)
    check_pair(plain, quant, fmt, "cuda", N // BS, 0 if case == "fixed" else 1)
