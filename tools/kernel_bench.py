#!/usr/bin/env python3
"""Device-resident throughput of the gfx950 collate kernels vs PyTorch's own kernels.

Inputs already live in HBM, so this measures the kernels alone (the loader's H2D is
measured by bench.py).  For each case it prints the device time per call (``gpu_us``:
calls captured in a HIP graph and replayed, so host launch cost is excluded) and the
effective HBM bandwidth (bytes read + bytes written) / time, next to the equivalent
PyTorch op (``Tensor.to`` for the cast, an index_put-based pad for var-len); ``eager_us``
is the wall time per eager call including the Python wrapper and launch.

``pack_rows`` (padded -> packed cu_seqlens layout, pack.hip) has no single PyTorch kernel to stand
beside: a boolean-mask gather synchronises with the host, so it cannot be graph-timed.

``mx_quantize`` (f32 / bf16 -> OCP MX blocks, mx_quant.hip) stands beside ``reference_mx``, the
plain-torch composition of the same rules, running on the same GPU; the two are timed alternately.

``struct_split`` (packed struct records -> one tensor per field, struct_split.hip) stands beside
``reference_struct``, the slice / view / to composition in plain torch, on the same device tensors.

Usage: python tools/kernel_bench.py [--quick] [--iters N] [--only pack_rows|mx_quantize|struct_split]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters  # µs


def timeit_graph(fn, iters, per_graph=20):
    """Device time per call: `per_graph` calls captured in one HIP graph, replayed, so the host's
    per-launch cost (Python wrapper + hipLaunchKernel) is out of the measurement."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    g.replay()
    torch.cuda.synchronize()
    reps = max(1, iters // per_graph)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / (reps * per_graph)


def pack_rows_cases(dev, iters):
    """Padded [256, 512] with lengths U(64, 512) -- benchmarks/varlen_tokens.py's batch -- packed by
    one launch: GPU time per launch and (kept elements read + capacity elements written, plus the
    lengths / cu_seqlens / ids traffic) / time.  ``eager_us``: wall time per ``pack_padded`` call (checks, pad
    bits, allocations, launch); ``loader_entry_us``: per ``pack_launch`` call, the loader's per-batch entry."""
    import torch

    from torchkafka_amd.ops.collate import pack_launch, pack_padded, pad_bits
    from torchkafka_amd.ops.native import hip

    mod = hip()
    g = torch.Generator().manual_seed(1)
    rows, W = 256, 512
    lens = torch.randint(64, W + 1, (rows,), generator=g)
    lens_d = lens.to(dev)
    total, cap = int(lens.sum()), rows * W
    res = []
    for name, dt, ids in (("256 rows, L~U(64,512) int64", torch.int64, False),
                          ("256 rows, L~U(64,512) bf16", torch.bfloat16, False),
                          ("256 rows, L~U(64,512) int64 + position/segment ids", torch.int64, True)):
        padded = torch.randint(0, 1 << 15, (rows, W), generator=g).to(dt).to(dev)
        esz = padded.element_size()
        values = torch.empty(cap, dtype=dt, device=dev)
        cu = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        tot = torch.empty((), dtype=torch.int64, device=dev)
        pos = torch.empty(cap, dtype=torch.int32, device=dev) if ids else None
        seg = torch.empty(cap, dtype=torch.int32, device=dev) if ids else None
        bits = pad_bits(dt, 0)

        def ours():
            mod.pack_rows(padded.data_ptr(), esz, rows, W, lens_d.data_ptr(), values.data_ptr(), cap, bits,
                          cu.data_ptr(), tot.data_ptr(), pos.data_ptr() if ids else 0, seg.data_ptr() if ids else 0,
                          torch.cuda.current_stream(dev).cuda_stream)

        ours()
        keep = torch.arange(W)[None, :] < lens[:, None]
        assert torch.equal(values[:total].cpu(), padded.cpu()[keep]) and int(tot) == total
        assert int(cu[-1]) == total and not bool(values[total:].any())
        nbytes = total * esz + cap * esz + rows * 8 + (rows + 1) * 4 + (2 * cap * 4 if ids else 0)
        g_ours = timeit_graph(ours, iters)
        t_op = timeit(lambda: pack_padded(padded, lens_d, None, 0, ids), iters)
        t_entry = timeit(lambda: pack_launch(padded, lens_d, cap, bits, ids), iters)  # what the loader calls per batch
        res.append({"kernel": "pack_rows", "case": name, "gpu_us": round(g_ours, 2),
                    "GBps": round(nbytes / g_ours / 1e3, 1), "padding_fraction": round(1 - total / cap, 3),
                    "eager_us": round(t_op, 2), "loader_entry_us": round(t_entry, 2)})
    return res


HBM_ROOF_GBPS = 6290.0  # measured float4 copy on MI355X (8 TB/s spec)


def mx_quantize_cases(dev, iters, rounds=3):
    """The config-2 batch (f32 [256, 256]), eight of them as one [2048, 256], and a [256, 2048] bf16
    token-feature batch -> mxfp8 and mxfp4.  ``gpu_us``: device time per launch (graph replay);
    ``GBps``: (input + values + scales bytes) / time and its share of the measured HBM roof;
    ``torch_gpu_us``: ``reference_mx`` on the same GPU, graph-replayed too (its launches back to back,
    no host gaps), the two alternated ``rounds`` times in this call (the median is reported, the
    spread kept); ``eager_us`` / ``torch_eager_us``: wall time per call with the host's launch cost."""
    import statistics

    import torch

    from torchkafka_amd.ops.collate import DTYPE_CODE, MX_FORMATS, mx_launch, quantize_mx, reference_mx
    from torchkafka_amd.ops.native import hip

    mod = hip()
    g = torch.Generator().manual_seed(2)
    res = []
    for name, shape, dt in (("config2 batch 256x256 f32", (256, 256), torch.float32),
                            ("8 config2 batches 2048x256 f32", (2048, 256), torch.float32),
                            ("token features 256x2048 bf16", (256, 2048), torch.bfloat16)):
        x = (torch.randn(shape, generator=g) * torch.exp2(torch.randint(-8, 8, shape, generator=g).float())).to(dt)
        x = x.to(dev)
        for fmt, code in MX_FORMATS.items():
            ours, ref = quantize_mx(x, fmt), reference_mx(x, fmt)
            assert torch.equal(ours.values.view(torch.uint8), ref.values.view(torch.uint8))
            assert torch.equal(ours.scales, ref.scales)
            nbytes = x.numel() * x.element_size() + ours.values.numel() + ours.scales.numel()
            values, scales = torch.empty_like(ours.values), torch.empty_like(ours.scales)

            def kernel():
                mod.mx_quantize(x.data_ptr(), DTYPE_CODE[dt], x.numel() // 32, code, values.data_ptr(),
                                scales.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)

            kernel()
            assert torch.equal(values.view(torch.uint8), ref.values.view(torch.uint8))
            assert torch.equal(scales, ref.scales)
            t_ours, t_ref = [], []
            for _ in range(rounds):  # alternated: other work shares the machine
                t_ours.append(timeit_graph(kernel, iters))
                t_ref.append(timeit_graph(lambda: reference_mx(x, fmt), iters))
            g_ours, g_ref = statistics.median(t_ours), statistics.median(t_ref)
            e_ours = timeit(lambda: quantize_mx(x, fmt), iters)
            e_ref = timeit(lambda: reference_mx(x, fmt), iters)
            t_entry = timeit(lambda: mx_launch(x, code, fmt), iters)  # what the loader calls per batch
            res.append({"kernel": "mx_quantize", "case": f"{name} -> {fmt}", "gpu_us": round(g_ours, 2),
                        "gpu_us_rounds": [round(t, 2) for t in t_ours], "bytes": nbytes,
                        "GBps": round(nbytes / g_ours / 1e3, 1),
                        "hbm_roof_share": round(nbytes / g_ours / 1e3 / HBM_ROOF_GBPS, 4),
                        "torch_gpu_us": round(g_ref, 2), "torch_gpu_us_rounds": [round(t, 2) for t in t_ref],
                        "eager_us": round(e_ours, 2), "torch_eager_us": round(e_ref, 2),
                        "loader_entry_us": round(t_entry, 2)})
    return res


def struct_split_cases(dev, iters, rounds=3):
    """Three struct batches -> their field tensors by one launch (struct_split.hip): the README
    struct (256 x 308 B, five fields), 256 x 1 KiB with four fields, 4096 x 64 B with eight scalar
    fields.  ``gpu_us``: device time per launch (graph replay); ``GBps``: (record bytes read + field
    bytes written) / time and its share of the measured HBM roof; ``torch_gpu_us``:
    ``reference_struct`` on the same device tensors -- the slice / view / to composition a user would
    write -- graph-replayed too, the two alternated ``rounds`` times (median reported, spread kept);
    ``eager_us`` / ``torch_eager_us``: wall time per call with the host's launch cost."""
    import statistics

    import torch

    from torchkafka_amd import Field, Struct
    from torchkafka_amd.ops.collate import reference_struct, split_struct, struct_launch
    from torchkafka_amd.ops.native import hip

    mod = hip()
    f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
    u8, i8, i32, i64 = torch.uint8, torch.int8, torch.int32, torch.int64
    readme = Struct(Field("flag", u8), Field("features", f32, (64,), out=bf16, normalize=(0.5, 2.0)),
                    Field("ids", i32, (2, 4), out=i64), Field("weight", f16), Field("label", i64, offset=300), size=308)
    kib = Struct(Field("dense", f32, (192,), out=bf16, normalize=(0.0, 1.5)), Field("ids", i32, (48,), out=i64),
                 Field("weight", f32, offset=1012), Field("label", i64, offset=1016), size=1024)
    scalars = Struct(Field("a", f32), Field("b", f32, out=bf16), Field("c", i64), Field("d", i32, out=i64),
                     Field("e", f16, out=f32), Field("f", u8), Field("g", i8, out=i32, offset=27),
                     Field("h", bf16, offset=29), size=64)
    g = torch.Generator().manual_seed(3)
    res = []
    for name, schema, rows in (("README struct 256 x 308 B, 5 fields", readme, 256),
                               ("256 x 1 KiB, 4 fields", kib, 256),
                               ("4096 x 64 B, 8 scalar fields", scalars, 4096)):
        raw = torch.randint(0, 120, (rows, schema.size), dtype=u8, generator=g).to(dev)  # bytes < 0x78: no NaN
        ours, ref = split_struct(raw, schema), reference_struct(raw, schema)
        for f in schema.members:
            a, b = ours[f.name], ref[f.name]
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8)), f.name
        nbytes = raw.numel() + sum(t.numel() * t.element_size() for t in ours.values())
        outs = [torch.empty_like(ours[f.name]) for f in schema.members]
        spec = schema.device_spec(raw.device)
        table = [(off, f.elems, src, dst, o.data_ptr(), shift, scale)
                 for (off, _s, src, dst, shift, scale), f, o in zip(spec, schema.members, outs)]

        def kernel():
            mod.struct_split(raw.data_ptr(), rows, schema.size, table, torch.cuda.current_stream(dev).cuda_stream)

        kernel()
        for f, o in zip(schema.members, outs):
            assert torch.equal(o.view(torch.uint8), ours[f.name].view(torch.uint8)), f.name
        t_ours, t_ref = [], []
        for _ in range(rounds):  # alternated: other work shares the machine
            t_ours.append(timeit_graph(kernel, iters))
            t_ref.append(timeit_graph(lambda: reference_struct(raw, schema), iters))
        g_ours, g_ref = statistics.median(t_ours), statistics.median(t_ref)
        e_ours = timeit(lambda: split_struct(raw, schema), iters)
        e_ref = timeit(lambda: reference_struct(raw, schema), iters)
        t_entry = timeit(lambda: struct_launch(raw, schema), iters)  # what the loader calls per batch
        res.append({"kernel": "struct_split", "case": name, "gpu_us": round(g_ours, 2),
                    "gpu_us_rounds": [round(t, 2) for t in t_ours], "bytes": nbytes,
                    "tile_rows": int(mod.struct_tile_rows(rows, schema.size)),
                    "GBps": round(nbytes / g_ours / 1e3, 1),
                    "hbm_roof_share": round(nbytes / g_ours / 1e3 / HBM_ROOF_GBPS, 4),
                    "torch_gpu_us": round(g_ref, 2), "torch_gpu_us_rounds": [round(t, 2) for t in t_ref],
                    "eager_us": round(e_ours, 2), "torch_eager_us": round(e_ref, 2),
                    "loader_entry_us": round(t_entry, 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for counter collection)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default=None, choices=["pack_rows", "mx_quantize", "struct_split"],
                    help="run only this kernel's cases")
    args = ap.parse_args()
    iters = 20 if args.quick else args.iters

    import torch

    from torchkafka_amd.ops.collate import collate_fixed, collate_varlen
    from torchkafka_amd.ops.native import hip

    hip()
    dev = torch.device("cuda", 0)
    if args.only == "pack_rows":
        for r in pack_rows_cases(dev, iters):
            print(json.dumps(r))
        return
    if args.only == "mx_quantize":
        for r in mx_quantize_cases(dev, iters):
            print(json.dumps(r))
        return
    if args.only == "struct_split":
        for r in struct_split_cases(dev, iters):
            print(json.dumps(r))
        return
    out = []

    fixed_cases = [("config2 batch 256x256 f32->bf16", 256, 256, torch.bfloat16),
                   ("256x256 f32->fp8e4m3", 256, 256, torch.float8_e4m3fn),
                   ("bs1024 1024x256 f32->bf16", 1024, 256, torch.bfloat16),
                   ("config5 8x262144 f32->bf16 (8 MiB)", 8, 262144, torch.bfloat16),
                   ("64x262144 f32->bf16 (64 MiB)", 64, 262144, torch.bfloat16),
                   ("256x262144 f32->bf16 (256 MiB)", 256, 262144, torch.bfloat16)]
    for name, rows, row, dt in fixed_cases:
        src = torch.randn(rows, row, device=dev)
        t_ours = timeit(lambda: collate_fixed(src, dt), iters)
        t_torch = timeit(lambda: src.to(dt), iters)
        g_ours = timeit_graph(lambda: collate_fixed(src, dt), iters)
        g_torch = timeit_graph(lambda: src.to(dt), iters)
        nbytes = src.numel() * 4 + src.numel() * torch.empty((), dtype=dt).element_size()
        out.append({"kernel": "fixed", "case": name, "gpu_us": round(g_ours, 2),
                    "GBps": round(nbytes / g_ours / 1e3, 1),
                    "torch_gpu_us": round(g_torch, 2), "torch_GBps": round(nbytes / g_torch / 1e3, 1),
                    "eager_us": round(t_ours, 2), "torch_eager_us": round(t_torch, 2)})

    g = torch.Generator().manual_seed(0)
    var_cases = [("config4 256 rows, L~U(0,512) f32->bf16", 256, 512, torch.float32),
                 ("256 rows, L~U(0,8192) f32->bf16", 256, 8192, torch.float32),
                 ("4096 rows, L~U(0,4096) f32->bf16", 4096, 4096, torch.float32),
                 ("LDS-staged: 4096 rows, L~U(0,4096) bf16->bf16", 4096, 4096, torch.bfloat16)]
    src_code = {torch.float32: 0, torch.bfloat16: 2}
    for name, rows, lmax, sdt in var_cases:
        lens = torch.randint(0, lmax + 1, (rows,), generator=g)
        offs = torch.zeros(rows + 1, dtype=torch.int32)
        offs[1:] = lens.cumsum(0).to(torch.int32)
        vals = torch.randn(int(offs[-1]), device=dev).to(sdt)
        offs_d = offs.to(dev)
        L = int(lens.max())
        esz = vals.element_size()
        nbytes = vals.numel() * esz + rows * L * 2

        buf = torch.zeros(vals.numel() * esz + 64, dtype=torch.uint8, device=dev)
        buf[: vals.numel() * esz].copy_(vals.view(torch.uint8))
        o = torch.empty((rows, L), dtype=torch.bfloat16, device=dev)
        ln = torch.empty(rows, dtype=torch.int64, device=dev)
        mod = hip()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def ours():
            mod.collate_varlen(offs_d.data_ptr(), buf.data_ptr(), src_code[sdt], o.data_ptr(), 2, rows, L, 0.0,
                               ln.data_ptr(), 0, stream)

        row_idx = torch.repeat_interleave(torch.arange(rows, device=dev), lens.to(dev))
        col_idx = torch.arange(vals.numel(), device=dev) - offs_d[:-1].long().repeat_interleave(lens.to(dev))

        def torch_pad():
            t = torch.zeros((rows, L), dtype=torch.bfloat16, device=dev)
            t[row_idx, col_idx] = vals.to(torch.bfloat16)
            return t

        # numerics check once
        ours()
        assert torch.equal(o.view(torch.int16), torch_pad().view(torch.int16))
        _ = collate_varlen(offs_d, vals, torch.bfloat16, L=L)
        t_ours = timeit(ours, iters)
        t_torch = timeit(torch_pad, iters)
        g_ours = timeit_graph(lambda: mod.collate_varlen(offs_d.data_ptr(), buf.data_ptr(), src_code[sdt], o.data_ptr(),
                                                          2, rows, L, 0.0, ln.data_ptr(), 0,
                                                          torch.cuda.current_stream(dev).cuda_stream), iters)
        g_torch = timeit_graph(torch_pad, iters)
        out.append({"kernel": "varlen", "case": name, "gpu_us": round(g_ours, 2),
                    "GBps": round(nbytes / g_ours / 1e3, 1),
                    "torch_gpu_us": round(g_torch, 2), "torch_GBps": round(nbytes / g_torch / 1e3, 1),
                    "eager_us": round(t_ours, 2), "torch_eager_us": round(t_torch, 2)})

    # device JSON parse (json_parse.hip) from HBM: text bytes parsed per second, against the
    # workers' native host parser on the same rows (no PyTorch GPU equivalent exists)
    import random
    import time

    import numpy as np

    from torchkafka_amd.ops.native import core

    rnd = random.Random(0)
    for name, rows in (("config4 256 rows JSON -> bf16", 256), ("4096 rows JSON -> bf16", 4096)):
        texts = []
        for _ in range(rows):
            n = rnd.randint(16, 256)
            texts.append(("[" + ", ".join("%.2f" % rnd.uniform(-50, 51) for _ in range(n)) + "]").encode())
        desc = np.zeros((rows, 4), dtype=np.int32)
        blob = bytearray()
        for i, t in enumerate(texts):
            at = (len(blob) + 31) // 32 * 32
            blob.extend(b"\0" * (at - len(blob)))
            cnt = core().json_scan_simple(t)
            desc[i] = (at, len(t), cnt, cnt)
            blob.extend(t)
        blob.extend(b"\0" * 64)
        L = int(desc[:, 3].max())
        d_desc = torch.from_numpy(desc).to(dev)
        d_vals = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        o = torch.empty((rows, L), dtype=torch.bfloat16, device=dev)
        ln = torch.empty(rows, dtype=torch.int64, device=dev)
        mod = hip()

        def jparse():
            mod.launch_json_rows(d_desc.data_ptr(), d_vals.data_ptr(), o.data_ptr(), 2, rows, L, 0.0, ln.data_ptr(), 0,
                                 0, torch.cuda.current_stream(dev).cuda_stream)

        jparse()
        ref = torch.zeros((rows, L), dtype=torch.float32)
        for i, t in enumerate(texts):
            v = json.loads(t)
            ref[i, : len(v)] = torch.tensor(v, dtype=torch.float64).float()
        assert torch.equal(o.cpu().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
        g_ours = timeit_graph(jparse, iters)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            for t in texts:
                core().parse_json_f32(t)
        host_us = (time.perf_counter() - t0) / reps * 1e6
        text_bytes = sum(len(t) for t in texts)
        out.append({"kernel": "json_parse", "case": name, "gpu_us": round(g_ours, 2),
                    "text_GBps": round(text_bytes / g_ours / 1e3, 1), "numbers": int(desc[:, 2].sum()),
                    "host_parser_us_one_core": round(host_us, 1)})

    out += pack_rows_cases(dev, iters)
    out += mx_quantize_cases(dev, iters)
    out += struct_split_cases(dev, iters)
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
