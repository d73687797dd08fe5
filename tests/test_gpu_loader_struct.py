"""A Struct topic through every decode route of the GPU loader: dicts byte-equal to the loop oracle
over the produced bytes, a fixed order with ``in_order=True``, exact commits; and the int32 carrier
itself, which a plain ``FixedWidth`` loader over the same topic still delivers unchanged.

The topic is the 52-byte struct of ``helpers/structs.py`` in 3 partitions x 70 records with keys of
0-8 bytes, so every value's alignment in the log shifts; batch 32, so the last batch is partial."""
import pytest
import torch

from helpers import structs as S
from test_gpu_loader_reference import _dataset, _loader

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUTES = {
    "auto": {"decode": "auto"},
    "dma": {"h2d": "dma"},
    "host": {"decode": "host"},
    "coalesce4": {"coalesce": 4},
    "return_info": {"return_info": True},
}
COMMITTED = {0: 70, 1: 70, 2: 70}


def stamps_of(batches):
    return torch.cat([b["i"][:, 0].cpu() for b in batches]).tolist()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_struct_topic_through_a_route(broker, route):
    from torchkafka_amd import KafkaBatch, auto_commit

    s = S.struct52()
    rows = S.produce_struct(broker, s, seed=3)
    orders = []
    for run in range(2):  # twice, under two groups: in_order=True gives the same order both times
        dl = _loader(broker, _dataset(s), S.BS, DEV, f"g{run}", **ROUTES[route])
        items = list(auto_commit(dl))
        dl.close()
        if route == "return_info":
            assert all(isinstance(i, KafkaBatch) and i.lengths is None and i.mask is None for i in items)
            assert sum(i.n_records for i in items) == S.PARTS * S.PER_PART
            items = [i.data for i in items]
        S.check_batches(s, rows, items, "cuda")
        assert min(b["u"].shape[0] for b in items) < S.BS  # a partial batch was delivered
        assert broker.committed_offsets(f"g{run}", "t") == COMMITTED
        orders.append(stamps_of(items))
    assert orders[0] == orders[1]


def test_struct_topic_single_process_mode(broker):
    """num_workers=0: the dataset's own consumer, a packer thread in this process."""
    from torchkafka_amd import DeviceLoader, auto_commit

    s = S.struct52()
    rows = S.produce_struct(broker, s, seed=4)
    ds = _dataset(s)("t", bootstrap_servers=broker.url, group_id="g", auto_offset_reset="earliest",
                     consumer_timeout_ms=300)
    dl = DeviceLoader(ds, S.BS, num_workers=0, device=DEV, in_order=True)
    items = list(auto_commit(dl))
    dl.close()
    S.check_batches(s, rows, items, "cuda")
    assert broker.committed_offsets("g", "t") == COMMITTED


def test_the_carrier_is_still_delivered_unchanged(broker):
    """FixedWidth(int32) over the struct topic: the words of every record, and split_struct of
    those batches is what the Struct loader delivers."""
    from torchkafka_amd import FixedWidth, auto_commit, split_struct

    s = S.struct52()
    rows = S.produce_struct(broker, s, seed=5)
    dl = _loader(broker, _dataset(FixedWidth(torch.int32, (13,))), S.BS, DEV, "carrier")
    got = [x.clone() for x in auto_commit(dl)]
    dl.close()
    assert all(x.dtype == torch.int32 and x.shape[1:] == (13,) and x.device.type == "cuda" for x in got)
    words = torch.cat(got).cpu()
    order = torch.argsort(words.view(torch.uint8).view(-1, 52)[:, 35:39].contiguous().view(torch.int32).flatten())
    assert torch.equal(words[order].view(torch.uint8).view(-1, 52), torch.cat(rows))
    assert broker.committed_offsets("carrier", "t") == COMMITTED
    S.check_batches(s, rows, [split_struct(x, s) for x in got], "cuda")


def test_skip_bad_on_the_gpu(broker):
    from torchkafka_amd import auto_commit

    lax = S.struct52(skip_bad=True)
    rows = S.produce_struct(broker, lax, seed=6, bad_at=(2, 40))
    dl = _loader(broker, _dataset(lax), S.BS, DEV, "lax")
    items = list(auto_commit(dl))
    dl.close()
    S.check_batches(lax, rows, items, "cuda")
    assert broker.committed_offsets("lax", "t") == {0: 70, 1: 70, 2: 71}
