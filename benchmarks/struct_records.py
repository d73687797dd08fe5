#!/usr/bin/env python3
"""What the Struct post-pass costs end to end: a ``Struct`` loader over 1 KiB records against a
``FixedWidth(int32, (256,))`` loader -- the struct's own carrier, without the split launch -- over
the same topic, alternated ``--rounds`` times under fresh consumer groups.

The records are the synthetic broker's ``fixed_f32`` rows of 256 floats; the struct reads them as
192 float features (-> bfloat16, normalised), 48 int32 ids (-> int64), a float32 weight at byte 1012
and an int64 label at byte 1016.  Each timed run takes ``--steps`` batches after ``--warmup``, with
per-batch commits (``auto_commit``), and ends with a device synchronisation.

Usage: python benchmarks/struct_records.py [--steps K] [--rounds N] [--device cuda:0]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    import torch

    from torchkafka_amd import DeviceLoader, Field, FixedWidth, KafkaDataset, Struct, auto_commit
    from torchkafka_amd.broker import SyntheticBroker

    f32, i32, i64 = torch.float32, torch.int32, torch.int64

    class Events(KafkaDataset):
        schema = Struct(Field("dense", f32, (192,), out=torch.bfloat16, normalize=(0.0, 1.5)),
                        Field("ids", i32, (48,), out=i64), Field("weight", f32, offset=1012),
                        Field("label", i64, offset=1016), size=1024)

    class Carrier(KafkaDataset):
        schema = FixedWidth(i32, (256,))

    B = args.batch_size
    per_part = -(-(args.steps + args.warmup + 64) * B // args.partitions)
    url = f"shm://structbench-{os.getpid()}"
    broker = SyntheticBroker.create(url, log_capacity=max(1 << 30, int(per_part * 1100)),
                                    index_capacity=max(1 << 20, per_part))
    on_gpu = args.device.startswith("cuda")
    try:
        broker.create_topic("events", args.partitions)
        broker.fill("events", per_part, "fixed_f32", size=256, records_per_batch=512,
                    threads=min(16, args.partitions))

        def run(ds, group):
            dl = DeviceLoader(ds.placeholder(), B, num_workers=args.workers, device=args.device,
                              worker_init_fn=ds.init_worker("events", bootstrap_servers=url, group_id=group,
                                                            auto_offset_reset="earliest"))
            it = iter(auto_commit(dl))
            try:
                for _ in range(args.warmup):
                    next(it)
                if on_gpu:
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = 0
                for _ in range(args.steps):
                    x = next(it)
                    rows += (x["label"] if isinstance(x, dict) else x).shape[0]
                if on_gpu:
                    torch.cuda.synchronize()
                return rows / (time.perf_counter() - t0)
            finally:
                it.close()
                dl.close()

        rates = {"struct": [], "carrier": []}
        for r in range(args.rounds):  # alternated: other work shares the machine
            rates["carrier"].append(run(Carrier, f"carrier-{r}"))
            rates["struct"].append(run(Events, f"struct-{r}"))
        out = {"benchmark": "struct_records", "record_bytes": 1024, "batch_size": B, "steps": args.steps,
               "rounds": args.rounds, "device": args.device}
        for k, v in rates.items():
            out[k] = {"records_per_s": [round(x) for x in v], "median": round(statistics.median(v)),
                      "min": round(min(v)), "max": round(max(v))}
        out["struct_over_carrier"] = round(statistics.median(rates["struct"]) / statistics.median(rates["carrier"]), 4)
        print(json.dumps(out))
    finally:
        broker.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
