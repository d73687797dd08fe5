#!/usr/bin/env python3
"""Multi-field records: a packed struct per record value, a dict of tensors per batch.

The producer packs a flag byte, 64 float32 features, eight int32 ids, a float16 weight and an int64
label into every record value (little-endian, no alignment padding).  ``Struct`` declares that
layout; the loader moves the record as int32 words through its usual native path and one gfx950
launch behind the decode splits every batch into the per-field tensors, converting the features to
bfloat16 with a fused normalisation and widening the ids to int64 on the way.  On the CPU the same
batches come from plain torch.

    python examples/09_struct_records.py [--device cpu]   # cuda:0 when available, else CPU
"""
import argparse
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from torchkafka import DeviceLoader, Field, KafkaDataset, Struct, auto_commit  # noqa: E402
from torchkafka_amd.broker import SyntheticBroker  # noqa: E402

MEAN, STD = 0.5, 2.0


class Events(KafkaDataset):
    schema = Struct(
        Field("flag", torch.uint8),                                                   # offset 0
        Field("features", torch.float32, (64,), out=torch.bfloat16, normalize=(MEAN, STD)),  # offset 1: packed
        Field("ids", torch.int32, (2, 4), out=torch.int64),
        Field("weight", torch.float16),
        Field("label", torch.int64, offset=300),                                      # the gap before it is skipped
        size=308)


def record(i: int) -> bytes:
    feats = [(i % 97) * 0.25 + j for j in range(64)]
    body = struct.pack("<B64f8ie", i % 2, *feats, *(i * 8 + k for k in range(8)), 1.0 + (i % 4) * 0.5)
    return body.ljust(300, b"\0") + struct.pack("<q", i)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--records", type=int, default=1000)
    args = ap.parse_args()
    cluster = SyntheticBroker.create(f"shm://example9-{os.getpid()}")
    try:
        cluster.create_topic("events", 2)
        for p in range(2):
            cluster.produce("events", [record(i) for i in range(p, args.records, 2)], partition=p)
        loader = DeviceLoader(Events.placeholder(), 128, num_workers=2, device=args.device,
                              worker_init_fn=Events.init_worker("events", bootstrap_servers=cluster.url,
                                                                group_id="example9", auto_offset_reset="earliest",
                                                                consumer_timeout_ms=1000))
        n = bad = 0
        for batch in auto_commit(loader):
            label = batch["label"]
            want = (((label % 97).float() * 0.25 - MEAN) * (1.0 / STD)).to(torch.bfloat16)
            bad += int((batch["features"][:, 0] != want).sum())
            bad += int((batch["ids"][:, 0, 0] != label * 8).sum()) + int((batch["flag"] != label % 2).sum())
            n += label.shape[0]
        loader.close()
        shapes = {k: (str(v.dtype).replace("torch.", ""), tuple(v.shape[1:])) for k, v in batch.items()}
        print(f"{n} struct records on {args.device}, {bad} field mismatches; fields: {shapes}")
        print("committed offsets:", cluster.committed_offsets("example9", "events"))
    finally:
        cluster.destroy()


if __name__ == "__main__":
    main()
