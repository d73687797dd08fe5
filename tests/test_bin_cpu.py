"""The binned (first-fit) layout without a GPU: ``reference_binned``, the config refusals and the CPU
loader with ``layout="binned"``, against a Python loop over the rows and bins (tests/helpers/binned.py)."""
import pytest
import torch

from helpers.binned import binned_layout, check_binned
from helpers.known_records import expected_varlen, expected_width, known_values, produce_known
from test_gpu_loader_reference import (VAR_BS, VAR_N, VAR_RPB, VARLEN_CASES, _dataset, _loader, _seed, _varlen_rows)
from test_gpu_pack import _lengths

F32, BF16, FP8, U8, I64 = torch.float32, torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.int64
DTYPES = {"u8": U8, "bf16": BF16, "f32": F32, "i64": I64, "fp8": FP8}
SEQ = 256  # the loader tests' seq_len: most rows have 0..60 elements, the long ones are cut


def bin_counts(lens, W: int, seq_len: int, rows: int):
    """The ``bins`` cases: the default (None), 1, the number the default run used, half of that, rows + 3."""
    used = binned_layout(lens, W, seq_len, rows)["n_bins"]
    return [None] + sorted({1, used, used // 2, rows + 3} - {0})


@pytest.mark.parametrize("rows,W,seq_len", [(0, 9, 12), (1, 9, 12), (33, 0, 5), (33, 1, 1), (65, 9, 12), (65, 9, 5),
                                            (65, 7, 64)])
@pytest.mark.parametrize("name", list(DTYPES))
def test_reference_binned_matches_the_loop(name, rows, W, seq_len):
    from torchkafka_amd import reference_binned

    dt = DTYPES[name]
    padded = known_values(F32 if dt == FP8 else dt, rows * W, 11 * rows + W).to(dt).view(rows, W)
    lens = _lengths(rows, W, 31 * rows + W)
    pads = (-1, float("nan")) if dt == F32 else (-1,)
    for bins in bin_counts(lens, W, seq_len, rows):
        for pad in pads:
            bb = reference_binned(padded, torch.tensor(lens, dtype=torch.int64), seq_len, bins, pad)
            check_binned(bb, padded, lens, seq_len, rows if bins is None else bins, pad,
                         f"{name} {rows}x{W} seq_len {seq_len} bins {bins} pad {pad}")
    bb = reference_binned(padded, torch.tensor(lens, dtype=torch.int64), seq_len)  # default bins, pad 0
    check_binned(bb, padded, lens, seq_len, rows, 0, f"{name} {rows}x{W} default")


def test_the_shapes_reach_every_branch():
    """What the chosen shapes are there for (lengths from test_gpu_pack._lengths, as the GPU tests use)."""
    rows, W = 65, 9
    lens = _lengths(rows, W, 31 * rows + W)
    lay = binned_layout(lens, W, 12, rows)
    newest, back_filled = -1, 0
    for b, n in zip(lay["row_bin"], lay["row_lens"]):
        back_filled += n > 0 and b < newest
        newest = max(newest, b)
    assert lay["unplaced"] == 0 and lay["cut"] == 0 and lay["n_bins"] > 1 and back_filled > 0
    half = binned_layout(lens, W, 12, lay["n_bins"] // 2)
    first = half["row_bin"].index(-1)
    later = zip(half["row_bin"][first:], half["row_lens"][first:])
    assert half["unplaced"] > 0 and any(b >= 0 and n > 0 for b, n in later)
    assert binned_layout(lens, W, 5, rows)["cut"] > 0
    assert binned_layout(_lengths(257, 9, 31 * 257 + 9), 9, 9, 257)["n_bins"] > 64
    assert binned_layout(_lengths(1025, 9, 31 * 1025 + 9), 9, 64, 1025)["n_bins"] > 64


def test_bin_padded_on_cpu_tensors_clamps_lengths_out_of_range():
    from torchkafka_amd import bin_padded

    padded = known_values(I64, 5 * 4, 3).view(5, 4)
    lens = [-3, 8, 2, 0, 4]
    bb = bin_padded(padded, torch.tensor(lens), 6)  # CPU tensors: the reference
    check_binned(bb, padded, lens, 6, 5, 0, "clamped")
    assert bb.row_lens.tolist() == [0, 4, 2, 0, 4] and bb.row_bin.tolist() == [0, 0, 0, 0, 1]
    assert bb.row_start.tolist() == [0, 0, 4, 6, 0] and bb.bin_lens.tolist() == [6, 4, 0, 0, 0]
    assert (int(bb.n_bins), int(bb.unplaced), int(bb.cut)) == (2, 0, 0)
    bb = bin_padded(padded, torch.tensor(lens, dtype=torch.int32), 3, 2, -1)
    check_binned(bb, padded, lens, 3, 2, -1, "cut and unplaced")
    assert (int(bb.n_bins), int(bb.unplaced), int(bb.cut)) == (2, 1, 2) and bb.row_bin.tolist() == [0, 0, 1, 0, -1]


@pytest.mark.parametrize("args", [(0, None), (-2, None), (4, -1), (1 << 31, None)])
def test_reference_binned_refuses_bad_sizes(args):
    from torchkafka_amd import reference_binned

    with pytest.raises(ValueError):
        reference_binned(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), *args)


@pytest.mark.parametrize("opts,msg", [
    ({"layout": "binned"}, "seq_len"),
    ({"layout": "binned", "seq_len": 0}, "seq_len"),
    ({"layout": "binned", "seq_len": 1 << 31}, "seq_len"),
    ({"layout": "binned", "seq_len": 64, "bins": 0}, "bins"),
    ({"layout": "binned", "seq_len": 64, "bins": 16385}, "bins"),
    ({"layout": "binned", "seq_len": 64, "return_mask": True}, "return_mask"),
    ({"layout": "binned", "seq_len": 64, "pack_to": 128}, "pack_to needs layout='packed'"),
    ({"layout": "binned", "seq_len": 64, "return_ids": True}, "return_ids needs layout='packed'"),
    ({"seq_len": 64}, "seq_len"),
    ({"bins": 4}, "bins"),
    ({"layout": "packed", "seq_len": 64}, "seq_len"),
    ({"layout": "packed", "bins": 4}, "bins"),
    ({"layout": "padded", "seq_len": 64}, "seq_len"),
])
def test_config_refuses(opts, msg):
    from torchkafka_amd import LoaderConfig

    with pytest.raises(ValueError, match=msg):
        LoaderConfig(**opts)
    with pytest.raises(ValueError, match=msg):
        LoaderConfig.build(None, **opts)


def test_config_accepts_binned():
    from torchkafka_amd import LoaderConfig

    cfg = LoaderConfig.build(None, layout="binned", seq_len=2048, bins=16384)
    assert (cfg.layout, cfg.seq_len, cfg.bins) == ("binned", 2048, 16384)
    assert LoaderConfig().seq_len is None and LoaderConfig().bins is None
    assert LoaderConfig(layout="binned", seq_len=1).bins is None
    back = LoaderConfig.from_dict(cfg.to_dict())
    assert (back.layout, back.seq_len, back.bins) == ("binned", 2048, 16384)


def test_binned_on_a_fixed_width_or_tree_schema_is_refused_at_construction():
    from torchkafka_amd import DeviceLoader, FixedWidth

    for schema in (FixedWidth(F32, (4,)), None):
        DS = _dataset(schema)
        with pytest.raises(TypeError, match="binned"):
            DeviceLoader(DS.placeholder(), 4, num_workers=1, device="cpu", layout="binned", seq_len=64,
                         worker_init_fn=DS.init_worker("t", bootstrap_servers="shm://nowhere", group_id="g"))


def binned_run(broker, case, device, seq_len=SEQ, **kw):
    """The var-len table ``case`` through DeviceLoader(layout='binned'): (loader, its batches, rows)."""
    from torchkafka_amd import VarLen, auto_commit

    src, dst, opts, max_len, _long = VARLEN_CASES[case]
    opts = {k: v for k, v in opts.items() if k != "return_mask"}
    rows = _varlen_rows(case)
    assert produce_known(broker, "t", rows, VAR_RPB, _seed(case) + 1) == VAR_N
    dl = _loader(broker, _dataset(VarLen(src, max_len=max_len)), VAR_BS, device, "g", dtype=dst, layout="binned",
                 seq_len=seq_len, **opts, **kw)
    got = [b for b in auto_commit(dl)]
    assert broker.committed_offsets("g", "t") == {0: VAR_N}  # cut and unplaced rows are committed too
    return dl, got, rows


def check_binned_run(case, got, rows, seq_len=SEQ, bins=None, drop_last=False):
    """Every delivered batch against expected_varlen + the loop; returns the expected layouts."""
    src, dst, opts, max_len, _long = VARLEN_CASES[case]
    n_batches = VAR_N // VAR_BS if drop_last else (VAR_N + VAR_BS - 1) // VAR_BS
    assert len(got) == n_batches
    seen = []
    for b, item in enumerate(got):
        if hasattr(item, "data"):  # return_info=True
            assert item.lengths is None and item.mask is None
            item = item.data
        part = rows[b * VAR_BS:(b + 1) * VAR_BS]
        L = expected_width([r.numel() for r in part], opts.get("pad_to"), opts.get("pad_multiple", 8), max_len)
        w_out, w_len, _mask = expected_varlen(part, dst, L, opts.get("pad_value", 0), max_len)
        seen.append(check_binned(item, w_out, w_len.tolist(), seq_len, len(part) if bins is None else bins,
                                 opts.get("pad_value", 0), f"{case} batch {b}", moved=False))
    return seen


@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_cpu_loader_delivers_the_expected_binned_batches(broker, case):
    _dl, got, rows = binned_run(broker, case, "cpu")
    seen = check_binned_run(case, got, rows)
    assert all(lay["unplaced"] == 0 for lay in seen)  # the default, a bin per row, leaves nothing out
    assert any(1 < lay["n_bins"] < len(lay["row_bin"]) for lay in seen)  # rows do share bins
    if VARLEN_CASES[case][2].get("pad_to") is None:
        assert any(lay["cut"] > 0 for lay in seen)  # the batches with a long row


def test_cpu_loader_with_too_few_bins_leaves_rows_out_and_still_commits_them(broker):
    case = "i64-i32-mask"
    _dl, got, rows = binned_run(broker, case, "cpu", seq_len=64, bins=3, return_info=True)  # asserts the commit
    seen = check_binned_run(case, got, rows, seq_len=64, bins=3)
    assert any(lay["unplaced"] > 0 for lay in seen)
    assert sum(b.n_records for b in got) == VAR_N
    for item, lay in zip(got, seen):
        assert tuple(item.data.values.shape) == (3, 64)
        assert int((item.data.row_bin < 0).sum()) == lay["unplaced"] == int(item.data.unplaced)
