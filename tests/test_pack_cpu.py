"""The packed (cu_seqlens) layout without a GPU: ``reference_packed``, the config refusals and the
CPU loader with ``layout="packed"``, against a Python loop over the rows (tests/helpers/packed.py)."""
import random

import pytest
import torch

from helpers.known_records import expected_varlen, expected_width, known_values, produce_known
from helpers.packed import capacities, check_packed
from test_gpu_loader_reference import (VAR_BS, VAR_N, VAR_RPB, VARLEN_CASES, _dataset, _loader, _seed, _varlen_rows)

F32, BF16, FP8, U8, I64 = torch.float32, torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.int64
DTYPES = {"u8": U8, "bf16": BF16, "f32": F32, "i64": I64, "fp8": FP8}


def length_sets(rows: int, W: int, seed: int):
    """Random lengths holding 0 and W (the last row full: capacity total - 1 cuts inside it), all 0, all W."""
    rng = random.Random(seed)
    mixed = [rng.randint(0, W) for _ in range(rows)]
    if rows:
        mixed[0], mixed[-1] = 0, W
    if rows > 2:
        mixed[rows // 2] = W
    return {"mixed": mixed, "zeros": [0] * rows, "full": [W] * rows}


@pytest.mark.parametrize("W", [0, 1, 9])
@pytest.mark.parametrize("rows", [0, 1, 33])
@pytest.mark.parametrize("name", list(DTYPES))
def test_reference_packed_matches_the_row_loop(name, rows, W):
    from torchkafka_amd import reference_packed

    dt = DTYPES[name]
    # every element known, the padding included: a read from the wrong place shows
    padded = known_values(F32 if dt == FP8 else dt, rows * W, 11 * rows + W).to(dt).view(rows, W)
    pads = (-1, float("nan")) if dt.is_floating_point else (-1,)
    for which, lens in length_sets(rows, W, rows + 7 * W).items():
        for cap in capacities(lens, W):
            for pad in pads:
                for ids in (False, True):
                    pb = reference_packed(padded, torch.tensor(lens, dtype=torch.int64), cap, pad, ids)
                    check_packed(pb, padded, lens, cap, pad, ids, f"{name} {rows}x{W} {which} cap {cap} pad {pad}")
        pb = reference_packed(padded, torch.tensor(lens, dtype=torch.int64))  # default: rows * W, pad 0
        check_packed(pb, padded, lens, rows * W, 0, False, f"{name} {rows}x{W} {which} default")


def test_reference_packed_clamps_lengths_out_of_range():
    from torchkafka_amd import pack_padded

    padded = known_values(I64, 5 * 4, 3).view(5, 4)
    lens = [-3, 8, 2, 0, 4]
    pb = pack_padded(padded, torch.tensor(lens), return_ids=True)  # CPU tensors: the reference
    check_packed(pb, padded, lens, 20, 0, True, "clamped")
    assert pb.cu_seqlens.tolist() == [0, 0, 4, 6, 6, 10]


@pytest.mark.parametrize("opts,msg", [
    ({"layout": "ragged"}, "layout"),
    ({"layout": "packed", "return_mask": True}, "return_mask"),
    ({"pack_to": 128}, "pack_to"),
    ({"return_ids": True}, "return_ids"),
    ({"layout": "padded", "pack_to": 128}, "pack_to"),
    ({"layout": "padded", "return_ids": True}, "return_ids"),
    ({"layout": "packed", "pack_to": 0}, "pack_to"),
    ({"layout": "packed", "pack_to": -4}, "pack_to"),
])
def test_config_refuses(opts, msg):
    from torchkafka_amd import LoaderConfig

    with pytest.raises(ValueError, match=msg):
        LoaderConfig(**opts)
    with pytest.raises(ValueError, match=msg):
        LoaderConfig.build(None, **opts)


def test_config_accepts_packed():
    from torchkafka_amd import LoaderConfig

    cfg = LoaderConfig.build(None, layout="packed", pack_to=4096, return_ids=True)
    assert (cfg.layout, cfg.pack_to, cfg.return_ids) == ("packed", 4096, True)
    assert LoaderConfig().layout == "padded" and LoaderConfig().pack_to is None and not LoaderConfig().return_ids
    assert LoaderConfig.from_dict(cfg.to_dict()).layout == "packed"


def test_packed_on_a_fixed_width_or_tree_schema_is_refused_at_construction():
    from torchkafka_amd import DeviceLoader, FixedWidth, KafkaDataset

    for schema in (FixedWidth(F32, (4,)), None):
        DS = _dataset(schema)
        with pytest.raises(TypeError, match="packed"):
            DeviceLoader(DS.placeholder(), 4, num_workers=1, device="cpu", layout="packed",
                         worker_init_fn=DS.init_worker("t", bootstrap_servers="shm://nowhere", group_id="g"))
    assert KafkaDataset.schema is None


def packed_run(broker, case, device, **kw):
    """The var-len table ``case`` through DeviceLoader(layout='packed'): (loader, its batches, rows)."""
    from torchkafka_amd import VarLen, auto_commit

    src, dst, opts, max_len, _long = VARLEN_CASES[case]
    opts = {k: v for k, v in opts.items() if k != "return_mask"}
    rows = _varlen_rows(case)
    assert produce_known(broker, "t", rows, VAR_RPB, _seed(case) + 1) == VAR_N
    dl = _loader(broker, _dataset(VarLen(src, max_len=max_len)), VAR_BS, device, "g", dtype=dst, layout="packed",
                 **opts, **kw)
    got = [b for b in auto_commit(dl)]
    assert broker.committed_offsets("g", "t") == {0: VAR_N}
    return dl, got, rows


def check_packed_run(case, got, rows, pack_to=None, ids=False, drop_last=False):
    """Every delivered batch against expected_varlen + the row loop; returns the (total, capacity) pairs."""
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
        cap = len(part) * L if pack_to is None else pack_to
        check_packed(item, w_out, w_len.tolist(), cap, opts.get("pad_value", 0), ids, f"{case} batch {b}",
                     moved=False)
        assert item.values.numel() == cap
        seen.append((int(item.total), cap))
    return seen


@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_cpu_loader_delivers_the_expected_packed_batches(broker, case):
    _dl, got, rows = packed_run(broker, case, "cpu")
    seen = check_packed_run(case, got, rows)
    assert all(total <= cap for total, cap in seen)  # the default capacity never cuts


def test_cpu_loader_pack_to_cuts_and_reports_the_overflow(broker):
    case = "i64-i64-default"
    _dl, got, rows = packed_run(broker, case, "cpu", pack_to=4096, return_ids=True)
    seen = check_packed_run(case, got, rows, pack_to=4096, ids=True)
    assert any(total > cap for total, cap in seen) and any(total <= cap for total, cap in seen)
    for item, (total, cap) in zip(got, seen):
        assert int(item.cu_seqlens[-1]) == min(total, cap)


def test_padded_layout_given_explicitly_is_the_default(broker):
    from torchkafka_amd import VarLen, auto_commit

    case = "i64-i32-mask"
    src, dst, opts, max_len, _long = VARLEN_CASES[case]
    rows = _varlen_rows(case)
    assert produce_known(broker, "t", rows, VAR_RPB, _seed(case) + 1) == VAR_N
    runs = []
    for group, kw in (("g0", {}), ("g1", {"layout": "padded"})):
        dl = _loader(broker, _dataset(VarLen(src, max_len=max_len)), VAR_BS, "cpu", group, dtype=dst, **opts, **kw)
        assert dl.layout == "padded" and dl.pack_to is None and dl.return_ids is False
        runs.append(list(auto_commit(dl)))
    assert len(runs[0]) == len(runs[1]) == 3
    for a, b in zip(*runs):
        assert type(a) is tuple and type(b) is tuple and len(a) == len(b) == 3
        for x, y in zip(a, b):
            assert type(x) is type(y) and x.dtype == y.dtype and torch.equal(x, y)
