"""DeviceLoader delivery paths against expected values built from the produced bytes.

Every other loader-path GPU test compares two of the project's own paths on random bytes; here each
path (the kernels it must reach: launch_fixed through the engine, fixed_group_kernel from pinned and
from staged memory, gather_fixed_kernel, span_decode_kernel from the pinned logs and from the HBM
mirror, the varlen collate kernel, varlen_span_kernel) is compared bit for bit with plain torch on
the CPU (tests/helpers/known_records.py), on known record contents: float specials and rounding
ties, full-range integers, and a per-feature normalisation that no two features share.

The same case tables run through ``DeviceLoader(device="cpu")`` in tests that need no GPU: they prove
the byte generation, the row order and the batch boundaries of this harness.
"""
import pytest
import torch

from helpers.known_records import (assert_same, assert_within_f32_bound, check_norm_vectors, esize, expected_fixed,
                                   expected_varlen, expected_width, known_rows, known_values, norm_vectors,
                                   produce_known)

F32, BF16, F16, FP8 = torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn
U8, I8, I32, I64 = torch.uint8, torch.int8, torch.int32, torch.int64

# name: (src, dst, shape, normalise, records, records per RecordBatch, batch size)
# Small rows: 103 records in batches of 32 -- three full batches (the second and third are staged
# together: a group launch) and a ragged last one, batch boundaries inside the 7-record RecordBatches.
FIXED_CASES = {
    # 52-byte rows: partial last 16-byte group, the gather's partial lane; denormals must survive
    "f32-f32-13-norm": (F32, F32, (13,), True, 103, 7, 32),
    # G = 31 and G = 32 16-byte groups per row: either side of span_decode's row-wave switch
    "f32-bf16-124-norm": (F32, BF16, (124,), True, 103, 7, 32),
    "f32-bf16-128-norm": (F32, BF16, (128,), True, 103, 7, 32),
    # 1056-byte rows: the gather's second 1 KiB wave segment; row % 8 == 0: the vector group kernel
    "f32-bf16-264-norm": (F32, BF16, (264,), True, 103, 7, 32),
    # G = 130 > 128: the wide-row mode of for_rows
    "f32-fp8-520": (F32, FP8, (520,), False, 103, 7, 32),
    # 16 000-byte rows: groups of one row owned by different LDS windows
    "f32-f16-4000-norm": (F32, F16, (4000,), True, 24, 5, 8),
    # 192 KB RecordBatches over 128 KiB segments: groups cut at a segment edge
    "f32-bf16-12000-norm": (F32, BF16, (12000,), True, 12, 4, 8),
    "bf16-f32-40-norm": (BF16, F32, (40,), True, 103, 7, 32),     # 2-byte source
    "f16-bf16-24": (F16, BF16, (24,), False, 103, 7, 32),         # 2-byte source with specials
    "u8-f16-48-norm": (U8, F16, (48,), True, 103, 7, 32),         # 1-byte source, 16 elements per group
    "u8-bf16-50-norm": (U8, BF16, (50,), True, 103, 7, 32),       # 1-byte source with a short tail
    "i8-f32-33": (I8, F32, (33,), False, 103, 7, 32),             # signed 1-byte source
    "i32-i64-3": (I32, I64, (3,), False, 3300, 400, 1000),        # many rows per segment
    "i64-i32-5": (I64, I32, (5,), False, 103, 7, 32),             # 8-byte source, wraps as Tensor.to wraps
    "i64-f32-5-norm": (I64, F32, (5,), True, 103, 7, 32),         # 8-byte source into the float path
    "i64-f32-1-norm": (I64, F32, (1,), True, 103, 7, 32),
}

# path: (DeviceLoader options, the kernel it must reach)
PATHS = {
    "copy1": dict(decode="host", h2d="zerocopy", coalesce=1),     # launch_fixed through the engine
    "copy4": dict(decode="host", h2d="zerocopy", coalesce=4),     # fixed_group_kernel
    "staged4": dict(decode="host", h2d="dma", coalesce=4),        # fixed_group_kernel, HBM source
    "direct": dict(h2d="direct", coalesce=4),                     # gather_fixed_kernel
    "span": dict(decode="device"),                                # span_decode_kernel
    "mirror": dict(decode="device", h2d="dma"),                   # span_decode_kernel, HBM mirror
}
EVERY_CASE_ON = ("span", "direct", "copy4")
# the other three paths: the 52-byte rows, the two-segment rows, the 1-byte short tail, every 8-byte source
ALSO_ON = {p: ("f32-f32-13-norm", "f32-bf16-264-norm", "u8-bf16-50-norm", "i64-i32-5", "i64-f32-5-norm",
               "i64-f32-1-norm") for p in ("copy1", "staged4", "mirror")}
# (case, path) pairs PathPlan refuses by design: (case, path) -> the refusing message.  None does.
REFUSED: dict = {}

MATRIX = [(c, p) for p in EVERY_CASE_ON for c in FIXED_CASES] + [(c, p) for p, cs in ALSO_ON.items() for c in cs]


def _dataset(schema):
    from torchkafka_amd import KafkaDataset

    class DS(KafkaDataset):
        pass

    DS.schema = schema
    return DS


def _seed(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 9973


def _fixed_setup(broker, case):
    src, dst, shape, norm, n, rpb, bs = FIXED_CASES[case]
    rows = known_rows(src, shape, n, _seed(case))
    assert produce_known(broker, "t", rows, rpb, _seed(case) + 1) == n
    mean = std = None
    if norm:
        mean, std = norm_vectors(rows[0].numel(), _seed(case))
        check_norm_vectors(mean, std)
    want = expected_fixed(rows, dst, mean, std)
    if norm and dst == F32:
        assert_within_f32_bound(want, rows, mean, std, "the plain-torch expected value")  # the bound holds at all
    return rows, want, mean, std


def _loader(broker, DS, bs, device, group, **kw):
    from torchkafka_amd import DeviceLoader

    return DeviceLoader(DS.placeholder(), bs, num_workers=1, device=device, in_order=True,
                        worker_init_fn=DS.init_worker("t", bootstrap_servers=broker.url, group_id=group,
                                                      auto_offset_reset="earliest", consumer_timeout_ms=300), **kw)


def _check_fixed(case, got, rows, want, mean, std):
    src, dst, shape, norm, n, rpb, bs = FIXED_CASES[case]
    assert [g.shape[0] for g in got] == [min(bs, n - i) for i in range(0, n, bs)]  # the batch boundaries
    out = torch.cat(got)
    assert_same(out, want, case)
    if norm and dst == F32:
        assert_within_f32_bound(out, rows, mean, std, case)


# ----------------------------------------------------------------------------- the harness itself (no GPU)
@pytest.mark.parametrize("row", sorted({1, 8} | {s[2][0] for s in FIXED_CASES.values()}))
def test_norm_vectors_distinguish_neighbouring_features(row):
    for seed in (0, 1, 77):
        mean, std = norm_vectors(row, seed)
        assert mean.shape == std.shape == (row,)
        check_norm_vectors(mean, std)


def test_known_rows_cover_specials_and_full_range():
    x = known_rows(F32, (13,), 103, 5)
    assert x.shape == (103, 13) and torch.equal(x.view(I32), known_rows(F32, (13,), 103, 5).view(I32))
    flat = x.flatten()
    assert bool(torch.isnan(flat).any()) and bool(torch.isinf(flat).any())
    assert bool(((flat != 0) & (flat.abs() < 2.0 ** -126)).any())  # f32 denormals
    assert bool((flat.view(I32) == -0x80000000).any())            # -0.0
    for dt in (U8, I8, I32, I64):
        v = known_values(dt, 400, 3)
        info = torch.iinfo(dt)
        assert int(v.min()) == info.min and int(v.max()) == info.max
    for dt in (I32, I64):
        v = set(known_values(dt, 400, 3).tolist())
        assert {(1 << 24) + 1, -(1 << 24) - 1, (1 << 24) + 3, -(1 << 24) - 3} <= v


@pytest.mark.parametrize("case", list(FIXED_CASES))
def test_cpu_loader_delivers_the_expected_fixed_batches(broker, case):
    """The case table through DeviceLoader(device='cpu'): bit-exact without normalisation, within
    the derived f32 bound with it (and bit-exact there too: the CPU loader evaluates the documented
    formula)."""
    from torchkafka_amd import FixedWidth, auto_commit

    src, dst, shape, norm, n, rpb, bs = FIXED_CASES[case]
    rows, want, mean, std = _fixed_setup(broker, case)
    dl = _loader(broker, _dataset(FixedWidth(src, shape)), bs, "cpu", "g", dtype=dst,
                 normalize=(mean, std) if norm else None)
    got = [x.clone() for x in auto_commit(dl)]
    assert broker.committed_offsets("g", "t") == {0: n}
    _check_fixed(case, got, rows, want, mean, std)


# ----------------------------------------------------------------------------- fixed width on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case,path", MATRIX)
def test_loader_path_matches_expected(broker, case, path):
    from torchkafka_amd import FixedWidth, auto_commit

    if (case, path) in REFUSED:
        pytest.skip(REFUSED[(case, path)])
    src, dst, shape, norm, n, rpb, bs = FIXED_CASES[case]
    rows, want, mean, std = _fixed_setup(broker, case)
    dl = _loader(broker, _dataset(FixedWidth(src, shape)), bs, "cuda:0", "g", dtype=dst,
                 normalize=(mean, std) if norm else None, **PATHS[path])
    got = []
    for x in auto_commit(dl):
        assert x.is_cuda
        got.append(x.cpu())  # synchronises: meanwhile the worker publishes the batches that follow
    assert broker.committed_offsets("g", "t") == {0: n}
    # the intended path ran
    plan, st = dl.plan, dl.stats
    assert plan.span == (path in ("span", "mirror")) and plan.mirror == (path == "mirror")
    assert plan.direct == (path == "direct") and plan.fast_path
    if path in ("span", "direct"):
        assert st.log_bytes_registered > 0   # the kernel read the pinned logs
    if path == "mirror":
        assert dl.stats_summary()["mirror_copies"] > 0
    if path in ("copy1", "copy4", "staged4"):
        assert st.log_bytes_registered == 0 and plan.h2d == ("dma" if path == "staged4" else "zerocopy")
    if path == "copy1":
        assert st.groups == 0
    if path in ("copy4", "staged4") and n // bs >= 3:
        assert st.groups > 0                 # full batches 2 and 3 were collated by one launch
    _check_fixed(case, got, rows, want, mean, std)


def test_every_case_runs_on_the_required_paths():
    pairs = set(MATRIX)
    assert len(pairs) == len(MATRIX)
    for p in EVERY_CASE_ON:
        assert all((c, p) in pairs for c in FIXED_CASES)
    for p in PATHS:
        mine = [c for c, q in pairs if q == p and (c, q) not in REFUSED]
        assert any(FIXED_CASES[c][3] for c in mine), f"{p}: no normalised case"
        assert any(esize(FIXED_CASES[c][0]) == 8 for c in mine), f"{p}: no 8-byte source"


# ----------------------------------------------------------------------------- var-len
# name: (src, dst, loader options, schema max_len, a worker-copied long row)
VARLEN_CASES = {
    "i64-i64-default": (I64, I64, {}, None, True),
    "i64-i32-mask": (I64, I32, {"return_mask": True, "pad_value": -1}, None, True),
    "i32-i64-truncate": (I32, I64, {}, 1500, True),               # max_len below the longest rows
    "f32-bf16-multiple16": (F32, BF16, {"pad_multiple": 16}, None, False),
    "f32-fp8-pad128": (F32, FP8, {"pad_to": 128}, None, False),
    "f16-f32-mask": (F16, F32, {"return_mask": True, "pad_value": -1}, None, False),
    "u8-f16-default": (U8, F16, {}, None, False),
}
VAR_N, VAR_RPB, VAR_BS = 70, 7, 32


def _varlen_rows(case):
    import random

    from torchkafka_amd.ops.native import core

    src, dst, opts, max_len, long_row = VARLEN_CASES[case]
    rng = random.Random(_seed(case))
    lens = [rng.randint(0, 60) for _ in range(VAR_N)]
    # every edge length; the longest rows in different batches: 2047 in the first, 2048 (a multiple of
    # 8: no slack after it) in the second, 2049 in the ragged last one
    for i, k in {0: 0, 3: 1, 5: 7, 6: 8, 9: 9, 17: 2047, 40: 2048, 66: 2049, 68: 0}.items():
        lens[i] = k
    if long_row:  # longer than one device segment: the worker copies it into the slot
        lens[45] = core().VAR_SPAN_ROW_MAX // esize(src) + 37
    vals = known_values(src, sum(lens), _seed(case) + 2)
    rows, pos = [], 0
    for k in lens:
        rows.append(vals[pos:pos + k])
        pos += k
    return rows


def _check_varlen(case, got, rows):
    src, dst, opts, max_len, long_row = VARLEN_CASES[case]
    assert len(got) == (VAR_N + VAR_BS - 1) // VAR_BS
    for b, item in enumerate(got):
        part = rows[b * VAR_BS:(b + 1) * VAR_BS]
        L = expected_width([r.numel() for r in part], opts.get("pad_to"), opts.get("pad_multiple", 8), max_len)
        w_out, w_len, w_mask = expected_varlen(part, dst, L, opts.get("pad_value", 0), max_len)
        assert len(item) == (3 if opts.get("return_mask") else 2)
        assert_same(item[0], w_out, f"{case} batch {b}")
        assert item[1].dtype == torch.int64 and torch.equal(item[1].cpu(), w_len), f"{case} batch {b}: lengths"
        if opts.get("return_mask"):
            assert item[2].dtype == torch.bool and torch.equal(item[2].cpu(), w_mask), f"{case} batch {b}: mask"


def _varlen_run(broker, case, device, **kw):
    from torchkafka_amd import VarLen, auto_commit

    src, dst, opts, max_len, long_row = VARLEN_CASES[case]
    rows = _varlen_rows(case)
    assert produce_known(broker, "t", rows, VAR_RPB, _seed(case) + 1) == VAR_N
    dl = _loader(broker, _dataset(VarLen(src, max_len=max_len)), VAR_BS, device, "g", dtype=dst, **opts, **kw)
    got = [tuple(t.cpu() for t in b) for b in auto_commit(dl)]
    assert broker.committed_offsets("g", "t") == {0: VAR_N}
    return dl, got, rows


@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_cpu_loader_delivers_the_expected_varlen_batches(broker, case):
    _dl, got, rows = _varlen_run(broker, case, "cpu")
    _check_varlen(case, got, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_varlen_path_matches_expected(broker, case, decode):
    """decode='host': the workers' CSR pack + the varlen collate kernel; decode='device':
    varlen_span_kernel on the pinned logs.  Values, lengths and mask of every batch."""
    dl, got, rows = _varlen_run(broker, case, "cuda:0", decode=decode, coalesce=4)
    assert dl.plan.var_span == (decode == "device") and dl.plan.varlen_fast
    assert (dl.stats.log_bytes_registered > 0) == (decode == "device")
    _check_varlen(case, got, rows)
