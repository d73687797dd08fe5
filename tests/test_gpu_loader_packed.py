"""``DeviceLoader(layout="packed")`` on the GPU: every var-len delivery route (host CSR + collate
kernel, device decode from the pinned logs and from the HBM mirror, the JSON device parse, the slot
route of return_info / drop_last) followed by the pack kernel, against expected_varlen + a Python
loop over the rows."""
import json
import random

import pytest
import torch

from helpers.known_records import expected_varlen, expected_width
from helpers.packed import check_packed
from test_gpu_loader_reference import VAR_BS, VARLEN_CASES, _dataset, _loader
from test_pack_cpu import check_packed_run, packed_run

pytestmark = pytest.mark.gpu


def _on_gpu(got):
    for item in got:
        pb = item.data if hasattr(item, "data") else item
        assert pb.values.is_cuda and pb.cu_seqlens.is_cuda and pb.total.is_cuda


@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("case", list(VARLEN_CASES))
def test_packed_varlen_path_matches_expected(broker, case, decode):
    dl, got, rows = packed_run(broker, case, "cuda:0", decode=decode, coalesce=4)
    assert dl.plan.varlen_fast
    assert dl.plan.var_span == (decode == "device")
    _on_gpu(got)
    check_packed_run(case, got, rows)


def test_packed_from_the_hbm_mirror(broker):
    dl, got, rows = packed_run(broker, "f32-bf16-multiple16", "cuda:0", decode="device", h2d="dma", coalesce=4)
    assert dl.plan.varlen_fast and dl.plan.var_span and dl.plan.mirror
    _on_gpu(got)
    check_packed_run("f32-bf16-multiple16", got, rows)


def test_packed_static_shapes_with_pack_to_and_drop_last(broker):
    case = "i64-i64-default"
    dl, got, rows = packed_run(broker, case, "cuda:0", decode="device", pack_to=4096, drop_last=True,
                               return_ids=True)
    _on_gpu(got)
    seen = check_packed_run(case, got, rows, pack_to=4096, ids=True, drop_last=True)
    assert any(total > cap for total, cap in seen)  # the batch with the long row is cut
    shapes = {(tuple(b.values.shape), tuple(b.cu_seqlens.shape), tuple(b.position_ids.shape),
               tuple(b.segment_ids.shape)) for b in got}
    assert shapes == {((4096,), (VAR_BS + 1,), (4096,), (4096,))}


def test_packed_with_return_info(broker):
    from torchkafka_amd import KafkaBatch

    case = "u8-f16-default"
    dl, got, rows = packed_run(broker, case, "cuda:0", decode="host", return_info=True)
    assert all(isinstance(b, KafkaBatch) and b.lengths is None and b.mask is None for b in got)
    assert sum(b.n_records for b in got) == len(rows)
    _on_gpu(got)
    check_packed_run(case, got, rows)


def test_packed_json_device_parse(broker):
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
    dl = _loader(broker, _dataset(JsonArray()), bs, "cuda:0", "g", json_parse="device", layout="packed",
                 pad_value=-1, return_ids=True, coalesce=4)
    got = list(auto_commit(dl))
    assert broker.committed_offsets("g", "t") == {0: n}
    assert dl.plan.json_device and dl.plan.varlen_fast
    rows = [torch.tensor([float(x) for x in json.loads(t)], dtype=torch.float64).to(torch.float32) for t in texts]
    assert len(got) == (n + bs - 1) // bs
    for b, pb in enumerate(got):
        part = rows[b * bs:(b + 1) * bs]
        L = expected_width([r.numel() for r in part], None, 8, None)
        w_out, w_len, _mask = expected_varlen(part, torch.float32, L, -1, None)
        assert pb.values.is_cuda
        check_packed(pb, w_out, w_len.tolist(), len(part) * L, -1, True, f"json batch {b}", moved=False)
