"""``DeviceLoader(layout="binned")`` on the GPU: every var-len delivery route (host CSR + collate
kernel, device decode from the pinned logs and from the HBM mirror, the JSON device parse, the slot
route of return_info / drop_last) followed by the bin kernels, against expected_varlen + a Python
loop over the rows and bins."""
import json
import random

import pytest
import torch

from helpers.binned import check_binned
from helpers.known_records import expected_varlen, expected_width
from test_bin_cpu import binned_run, check_binned_run
from test_gpu_loader_reference import VAR_BS, VARLEN_CASES, _dataset, _loader

pytestmark = pytest.mark.gpu


def _on_gpu(got):
    for item in got:
        bb = item.data if hasattr(item, "data") else item
        assert all(t.is_cuda for t in bb if isinstance(t, torch.Tensor))


@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_binned_varlen_path_matches_expected(broker, case, decode):
    dl, got, rows = binned_run(broker, case, "cuda:0", decode=decode, coalesce=4)
    assert dl.plan.varlen_fast
    assert dl.plan.var_span == (decode == "device")
    _on_gpu(got)
    seen = check_binned_run(case, got, rows)
    assert all(lay["unplaced"] == 0 for lay in seen)


def test_binned_from_the_hbm_mirror(broker):
    dl, got, rows = binned_run(broker, "f32-bf16-multiple16", "cuda:0", decode="device", h2d="dma", coalesce=4)
    assert dl.plan.varlen_fast and dl.plan.var_span and dl.plan.mirror
    _on_gpu(got)
    check_binned_run("f32-bf16-multiple16", got, rows)


def test_binned_cuts_a_row_longer_than_seq_len(broker):
    case = "i64-i64-default"
    dl, got, rows = binned_run(broker, case, "cuda:0", seq_len=64, decode="device")
    _on_gpu(got)
    seen = check_binned_run(case, got, rows, seq_len=64)
    assert all(lay["cut"] > 0 for lay in seen)  # 2047, 2048 and 2049 elements: one such row in every batch
    assert all(int(item.cut) == lay["cut"] for item, lay in zip(got, seen))


def test_binned_static_shapes_with_bins_and_drop_last(broker):
    case = "i64-i64-default"
    dl, got, rows = binned_run(broker, case, "cuda:0", seq_len=64, bins=4, decode="device", drop_last=True)
    _on_gpu(got)
    seen = check_binned_run(case, got, rows, seq_len=64, bins=4, drop_last=True)
    assert any(lay["unplaced"] > 0 for lay in seen)
    shapes = {tuple(tuple(t.shape) for t in b if isinstance(t, torch.Tensor)) for b in got}
    assert shapes == {((4, 64), (4, 64), (4, 64), (4,), (VAR_BS,), (VAR_BS,), (VAR_BS,), (), (), ())}


def test_binned_with_return_info(broker):
    from torchkafka_amd import KafkaBatch

    case = "u8-f16-default"
    dl, got, rows = binned_run(broker, case, "cuda:0", decode="host", return_info=True)
    assert all(isinstance(b, KafkaBatch) and b.lengths is None and b.mask is None for b in got)
    assert sum(b.n_records for b in got) == len(rows)
    _on_gpu(got)
    check_binned_run(case, got, rows)


def test_binned_json_device_parse(broker):
    from torchkafka_amd import JsonArray, auto_commit

    rng = random.Random(40)
    n, bs = 103, 32
    texts = []
    for _ in range(n):
        vals = [round(rng.uniform(-1e4, 1e4), rng.randint(0, 6)) for _ in range(rng.randint(0, 40))]
        texts.append(("[" + ", ".join(repr(v) for v in vals) + "]").encode())
    broker.create_topic("t", 1)
    for i in range(0, n, 9):
        broker.produce("t", texts[i:i + 9], partition=0)
    dl = _loader(broker, _dataset(JsonArray()), bs, "cuda:0", "g", json_parse="device", layout="binned", seq_len=96,
                 pad_value=-1, coalesce=4)
    got = list(auto_commit(dl))
    assert broker.committed_offsets("g", "t") == {0: n}
    assert dl.plan.json_device and dl.plan.varlen_fast
    rows = [torch.tensor([float(x) for x in json.loads(t)], dtype=torch.float64).to(torch.float32) for t in texts]
    assert len(got) == (n + bs - 1) // bs
    _on_gpu(got)
    for b, bb in enumerate(got):
        part = rows[b * bs:(b + 1) * bs]
        L = expected_width([r.numel() for r in part], None, 8, None)
        w_out, w_len, _mask = expected_varlen(part, torch.float32, L, -1, None)
        lay = check_binned(bb, w_out, w_len.tolist(), 96, len(part), -1, f"json batch {b}", moved=False)
        assert lay["unplaced"] == 0 and lay["cut"] == 0 and 1 < lay["n_bins"] < len(part)
