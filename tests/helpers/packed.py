"""The expected packed (cu_seqlens) batch, built by a Python loop over the rows.

Nothing here calls ``reference_packed`` or the pack kernel: ``packed_layout`` walks the rows one by
one and writes down where every kept element lands, ``expected_packed`` moves the bits.
"""
import torch

from helpers.known_records import assert_same, bits


def pad_element(dtype: torch.dtype, pad=0) -> torch.Tensor:
    """One element holding the pad value, rounded as ``expected_varlen`` rounds it."""
    if dtype.is_floating_point:
        return torch.tensor(float(pad), dtype=torch.float32).to(dtype)
    return torch.tensor(int(pad), dtype=torch.int64).to(dtype)


def packed_layout(lens, W: int, cap: int):
    """(source index [cap] into the flattened padded batch, -1 in the tail; cu int32 [rows+1]; the
    unclamped total; position_ids; segment_ids) for rows of ``lens`` elements (clamped to 0..W)."""
    idx = torch.full((cap,), -1, dtype=torch.int64)
    pos = torch.zeros(cap, dtype=torch.int32)
    seg = torch.full((cap,), -1, dtype=torch.int32)
    cu, at, total = [0], 0, 0
    for r, k in enumerate(lens):
        k = max(0, min(int(k), W))
        total += k
        keep = min(k, cap - at)
        if keep:
            idx[at:at + keep] = r * W + torch.arange(keep)
            pos[at:at + keep] = torch.arange(keep, dtype=torch.int32)
            seg[at:at + keep] = r
        at += keep
        cu.append(at)
    return idx, torch.tensor(cu, dtype=torch.int32), total, pos, seg


def expected_packed(padded: torch.Tensor, lens, cap: int, pad=0):
    """(values [cap], cu_seqlens, total, position_ids, segment_ids) of a CPU ``padded`` [rows, W]."""
    rows, W = padded.shape
    idx, cu, total, pos, seg = packed_layout(lens, W, cap)
    flat = bits(padded.contiguous()).reshape(-1)
    vals = bits(pad_element(padded.dtype, pad).reshape(1)).repeat(cap)
    kept = idx >= 0
    vals[kept] = flat[idx[kept]]
    return vals.view(padded.dtype), cu, total, pos, seg


def check_packed(pb, padded: torch.Tensor, lens, cap: int, pad=0, ids: bool = False, what: str = "",
                 moved: bool = True) -> None:
    """``pb`` (a PackedBatch, on any device) against the loop, bit for bit (assert_same).  ``moved``:
    ``padded`` is the very tensor that was packed, so NaN payloads must survive too; a loader test
    passes False -- its ``padded`` is torch's CPU cast of the records, whose NaN bits differ from
    the decode kernels' (only NaN-ness is pinned there, as everywhere in known_records)."""
    from torchkafka_amd import PackedBatch

    assert isinstance(pb, PackedBatch), (what, type(pb))
    values, cu, total, pos, seg = expected_packed(padded, lens, cap, pad)
    assert pb.values.dim() == 1
    assert_same(pb.values, values, f"{what}: values")
    kept = int(cu[-1])
    if moved:
        assert torch.equal(bits(pb.values.cpu())[:kept], bits(values)[:kept]), f"{what}: NaN payloads changed"
    assert pb.cu_seqlens.dtype == torch.int32 and torch.equal(pb.cu_seqlens.cpu(), cu), (
        what, pb.cu_seqlens.tolist()[:12], cu.tolist()[:12])
    assert pb.total.dtype == torch.int64 and pb.total.dim() == 0, what
    assert int(pb.total) == total, (what, int(pb.total), total)
    assert type(pb.max_seqlen) is int and pb.max_seqlen == padded.shape[1], (what, pb.max_seqlen)
    if ids:
        assert pb.position_ids.dtype == torch.int32 and torch.equal(pb.position_ids.cpu(), pos), f"{what}: position_ids"
        assert pb.segment_ids.dtype == torch.int32 and torch.equal(pb.segment_ids.cpu(), seg), f"{what}: segment_ids"
    else:
        assert pb.position_ids is None and pb.segment_ids is None, what
    assert_same(pb.trim(), values[:min(total, cap)], f"{what}: trim()")


def capacities(lens, W: int):
    """The capacity cases: total, total - 1 (a cut inside a row when the last row is not empty), a
    row boundary in the middle, total + 5 (tail fill)."""
    clamped = [max(0, min(int(k), W)) for k in lens]
    total = sum(clamped)
    caps = {total, total + 5, sum(clamped[:len(clamped) // 2])}
    if total >= 1:
        caps.add(total - 1)
    return sorted(caps)
