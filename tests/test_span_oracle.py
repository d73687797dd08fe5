"""The span kernels' oracle (tests/helpers/span_oracle.py) on the CPU: the independent CRC32C
against the standard vectors, and the project's host mirrors of the device CRC stage
(``crc32c_span_emulate``, ``crc32c_shift_raw``) against that oracle over the length table the GPU
sweep uses (tests/test_gpu_span_kernels.py).  tests/test_span_decode.py compares the mirrors with
``core().crc32c`` only: the project's own tables on both sides.
"""
import pytest

from helpers import span_oracle as so
from torchkafka_amd.ops.native import core

# RFC 3720 B.4 and the usual check value
VECTORS = [
    (b"123456789", 0xE3069283),
    (b"", 0x00000000),
    (bytes(32), 0x8A9136AA),
    (b"\xff" * 32, 0x62A8AB43),
    (bytes(range(32)), 0x46DD794E),
    (bytes(range(31, -1, -1)), 0x113FDB5C),
]


def _table_ok(table) -> bool:
    """The known vectors, and every table entry against the bitwise register of its byte."""
    return (all(so.crc32c(m, table) == want for m, want in VECTORS)
            and all(so.crc32c_raw(bytes([b]), 0, table) == so.raw_bitwise(bytes([b])) for b in range(256)))


def test_oracle_known_vectors():
    for m, want in VECTORS:
        assert so.crc32c(m) == want, m
        assert so.crc32c_bitwise(m) == want, m
    assert len(so.TABLE) == 256 and so.TABLE[1] == 0xF26B8303 and so.TABLE[255] == 0xAD7D5351
    assert _table_ok(so.TABLE)


def test_oracle_check_notices_any_changed_table_entry():
    for i in range(256):
        t = list(so.TABLE)
        t[i] ^= 1 << (i % 32)
        assert not _table_ok(t), i


def test_oracle_raw_register_and_chain():
    data = so.sweep_data(700, 9)
    assert so.crc32c_raw(data, 0xFFFFFFFF) ^ 0xFFFFFFFF == so.crc32c(data)
    # the register is linear: a run cut anywhere chains back to the whole
    cuts = [0, 61, 62, 300, 700]
    parts = []
    for i in range(len(cuts) - 1):
        seg = data[cuts[i]:cuts[i + 1]]
        parts.append((so.segment_raw(seg, i == 0), len(seg) - (so.FRONT if i == 0 else 0)))
    assert so.chain(parts) == so.crc32c(data[so.FRONT:])


def test_log_builder_alignment_and_slack():
    lb = so.LogBuilder(3)
    placed = []
    for a in list(range(16)) + [5, 5, 0]:
        d = so.sweep_data(1 + 7 * a, 2)
        placed.append((lb.place(d, a), a, d))
    raw = lb.finish()
    ends = []
    for p, a, d in placed:
        o = p - lb.base
        assert o % 16 == a and raw[o:o + len(d)] == d
        assert o >= so.SLACK and o + len(d) + so.SLACK <= len(raw)
        assert all(o >= e + so.SLACK for e in ends)
        ends.append(o + len(d))
    assert lb.base > 1 << 32


def _cases():
    c = core()
    assert c.SPAN_SEG_MAX == 131072
    return so.sweep_cases(_hip().SPAN_WIN, c.SPAN_SEG_MAX)


@pytest.mark.parametrize("parts", [1, 2, 4, 8])
def test_span_emulate_matches_oracle_over_the_sweep(parts):
    c = core()
    for n, first, _last in _cases():
        data = so.sweep_data(n)
        got = c.crc32c_span_emulate(data, so.FRONT if first else 0, n, first, parts)
        assert got == so.sweep_raw(n, first), (n, first, parts)


def test_span_emulate_at_every_source_offset():
    """The host mirror takes its range out of a larger buffer; the device sweep places the same
    bytes at every ``address & 15``."""
    c = core()
    for n in (1, 5, 21, 61, 81, 10239, 10241):
        for a in range(16):
            data = so.sweep_data(n)
            buf = bytes(a) + data
            assert c.crc32c_span_emulate(buf, a, a + n, False) == so.sweep_raw(n, False), (n, a)


def test_shift_raw_matches_oracle():
    c = core()
    for raw in (0, 1, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF):
        for n in (0, 1, 3, 4, 20, 21, 40, 61, 10220, 10240, 18929, 131051, 131072, 149999):
            assert c.crc32c_shift_raw(raw, n) == so.crc32c_raw(bytes(n), raw), (raw, n)


def test_chain_as_the_driver_combines_it():
    """batch_verdicts.cpp: acc = shift_raw(acc, crc_len) ^ partial, per segment of a RecordBatch."""
    c = core()
    data = so.sweep_data(300_000, 4)
    cuts = [0, 131_072, 150_001, 150_001 + 131_072, 300_000]
    acc = 0
    for i in range(len(cuts) - 1):
        seg = data[cuts[i]:cuts[i + 1]]
        assert len(seg) <= c.SPAN_SEG_MAX
        crc_len = len(seg) - (so.FRONT if i == 0 else 0)
        acc = c.crc32c_shift_raw(acc, crc_len) ^ so.segment_raw(seg, i == 0)
    assert acc ^ 0xFFFFFFFF == so.crc32c(data[so.FRONT:])


# ----------------------------------------------------------------------------- what the launch functions reject
# Every call below must be refused (std::invalid_argument -> ValueError).  PTR is a made-up address,
# so every call passes dry_run=True: the binding runs its own checks and the launch functions'
# (check_span_decode / check_var_span) and never launches.  A check that goes missing later then
# shows as a red test here, on a machine with a GPU too, not as a kernel reading PTR.
PTR = 0x7000_0000_1000


def _hip():
    from torchkafka_amd.ops.native import hip

    return hip()


def _fixed_args(n_seg=1, nb=1, **over):
    a = dict(src=[PTR] * n_seg, log_pos=[4096] * n_seg, len=[100] * n_seg, flags=[0] * n_seg, crc=[0] * n_seg,
             row_begin=[0] * n_seg, row_end=[1] * n_seg, batch=[0] * n_seg, seg=list(range(n_seg)),
             out=[PTR] * nb, row_pos=[PTR] * nb, err=[PTR] * nb, partials=[PTR] * nb, ext_out=[0] * nb,
             ext_src=[0] * nb, ext_words=[0] * nb, row_elems=8, vec_store=False, tabs=PTR, parts=1, part_acc=0,
             src_dtype=0, dst_dtype=0, dry_run=True)
    a.update(over)
    return a


def _var_args(n_seg=1, nb=1, **over):
    a = dict(src=[PTR] * n_seg, log_pos=[4096] * n_seg, len=[100] * n_seg, flags=[0] * n_seg, crc=[0] * n_seg,
             row_begin=[0] * n_seg, row_end=[1] * n_seg, batch=[0] * n_seg, seg=list(range(n_seg)),
             out=[PTR] * nb, rows=[PTR] * nb, slot=[0] * nb, lengths=[0] * nb, mask=[0] * nb, err=[PTR] * nb,
             partials=[PTR] * nb, L=[16] * nb, trunc_len=[-1] * nb, aligned=[False] * nb, tabs=PTR, parts=1,
             part_acc=0, src_dtype=6, dst_dtype=7, dry_run=True)
    a.update(over)
    return a


FIXED_REJECTS = {
    "len 0": dict(len=[0]),
    "len past kSpanSegMax": dict(len=[131073]),
    "more than kSpanMaxSegRows rows": dict(row_end=[2049]),
    "row_end below row_begin": dict(row_begin=[2], row_end=[1]),
    "parts 3": dict(parts=3, part_acc=PTR),
    "parts 16": dict(parts=16, part_acc=PTR),
    "parts without accumulator words": dict(parts=2, part_acc=0),
    "misaligned accumulator words": dict(parts=2, part_acc=PTR + 4),
    "sequences of unequal length": dict(crc=[0, 0]),
    "batch sequences of unequal length": dict(err=[PTR, PTR]),
    "a batch the launch does not have": dict(batch=[1]),
    "no source": dict(src=[0]),
    "vec_store with a short last group": dict(row_elems=7, vec_store=True),
    "vec_store with rows that are no multiple of 16 bytes": dict(row_elems=4, dst_dtype=2, vec_store=True),
    "vec_store into a misaligned output": dict(out=[PTR + 4], vec_store=True),
    "CRC without tables": dict(flags=[4], tabs=0),
    "float records into an integer dtype": dict(dst_dtype=6),
    "shift without scale": dict(shift=PTR),
    "ext_words without ext_out": dict(ext_words=[3]),
}


@pytest.mark.parametrize("what", list(FIXED_REJECTS))
def test_launch_span_group_rejects(what):
    with pytest.raises(ValueError):
        _hip().launch_span_group(**_fixed_args(**FIXED_REJECTS[what]))


def test_launch_span_group_rejects_too_many_segments_or_batches():
    h = _hip()
    with pytest.raises(ValueError):
        h.launch_span_group(**_fixed_args(n_seg=h.MAX_LAUNCH_SEGS + 1))
    with pytest.raises(ValueError):
        h.launch_span_group(**_fixed_args(nb=h.MAX_GROUP + 1))
    with pytest.raises(ValueError):
        h.launch_var_span_group(**_var_args(n_seg=h.MAX_LAUNCH_SEGS + 1))
    with pytest.raises(ValueError):
        h.launch_var_span_group(**_var_args(nb=h.MAX_GROUP + 1))


VAR_REJECTS = {
    "len 0": dict(len=[0]),
    "len past kSpanSegMax": dict(len=[131073]),
    "more than kJsonSpanMaxSegRows rows": dict(row_end=[1025]),
    "parts 5": dict(parts=5, part_acc=PTR),
    "parts without accumulator words": dict(parts=8, part_acc=0),
    "sequences of unequal length": dict(seg=[0, 1]),
    "batch sequences of unequal length": dict(L=[16, 16]),
    "a batch the launch does not have": dict(batch=[3]),
    "no source": dict(src=[0]),
    "aligned path with 8-byte groups": dict(src_dtype=0, dst_dtype=2, aligned=[True]),
    "aligned path into a misaligned output": dict(out=[PTR + 8], aligned=[True]),
    "aligned path with rows that are no multiple of 16 bytes": dict(L=[3], src_dtype=6, dst_dtype=6, aligned=[True]),
    "host rows without a slot": dict(flags=[8], len=[0], src=[0]),
    "float records into an integer dtype": dict(src_dtype=0, dst_dtype=7),
}


@pytest.mark.parametrize("what", list(VAR_REJECTS))
def test_launch_var_span_group_rejects(what):
    with pytest.raises(ValueError):
        _hip().launch_var_span_group(**_var_args(**VAR_REJECTS[what]))
