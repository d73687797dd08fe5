"""The Struct schema without a GPU: construction and its refusals, the record layout, ``process``
and ``reference_struct`` against the loop oracle of ``helpers/structs.py``, the CPU loader end to
end (exact commits, ``skip_bad``), the torch DataLoader compat path, the loader-option refusals and
the example."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from helpers import structs as S
from helpers.structs import BF16, F16, F32, FP8, I8, I32, I64, U8
from test_gpu_loader_reference import _dataset, _loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def readme_struct():
    from torchkafka_amd import Field, Struct

    mean = torch.linspace(-1, 1, 64)
    std = torch.linspace(0.5, 3, 64)
    return Struct(Field("flag", U8), Field("features", F32, (64,), out=BF16, normalize=(mean, std)),
                  Field("ids", I32, (2, 4), out=I64), Field("weight", F16), Field("label", I64, offset=300), size=308)


# ----------------------------------------------------------------------------- construction
def test_exports():
    import torchkafka
    import torchkafka_amd
    from torchkafka_amd import ops

    for mod in (torchkafka, torchkafka_amd):
        assert mod.Struct is torchkafka_amd.models.schema.Struct and mod.Field is torchkafka_amd.models.schema.Field
    assert ops.split_struct is torchkafka_amd.split_struct and ops.reference_struct is torchkafka_amd.reference_struct


def test_layout_default_and_explicit_offsets_gaps_and_overlaps():
    from torchkafka_amd import Field, Struct

    s = readme_struct()
    assert s.offsets == (0, 1, 257, 289, 300) and s.size == 308
    assert [f.nbytes for f in s.members] == [1, 256, 32, 2, 8]
    # the default size is the end of the last field; a field after an explicit offset follows it
    s = Struct(Field("a", I32, offset=8), Field("b", I32), Field("c", F16, (2,)))
    assert s.offsets == (8, 12, 16) and s.size == 20
    # overlap: a union read two ways.  The default size is the end of the LAST field, which here lies
    # below an earlier field's end: size= has to be given
    union = (Field("wide", I64, (2,)), Field("lo", I32, offset=0), Field("bytes", U8, (4,), offset=0))
    s = Struct(*union, size=16)
    assert s.offsets == (0, 0, 0) and s.size == 16
    with pytest.raises(ValueError, match="below the end of a field"):
        Struct(*union)
    S.struct52()


def test_the_carrier_interface():
    from torchkafka_amd import FixedWidth

    s = readme_struct()
    c = FixedWidth(I32, (77,))
    assert s.kind == 0 and s.fields == () and s.dtype == I32 and s.shape == (77,)
    assert (s.row_elems, s.elem_size, s.row_bytes, s.skip_bad) == (77, 4, 308, False)
    assert s.native_spec() == c.native_spec()
    assert S.struct52(skip_bad=True).native_spec() == FixedWidth(I32, (13,), skip_bad=True).native_spec()
    assert not hasattr(s, "extras_spec")


@pytest.mark.parametrize("dt", [torch.float64, torch.int16, torch.bool, torch.uint16, FP8])
def test_field_dtype_refused(dt):
    from torchkafka_amd import Field

    with pytest.raises(TypeError, match="dtype must be one of"):
        Field("x", dt)


def test_field_out_refusals():
    from torchkafka_amd import Field

    for out in (torch.float64, U8, I8, torch.int16):
        with pytest.raises(TypeError, match="out must be"):
            Field("x", I32, out=out)
    for src in (F32, F16, BF16):
        for out in (I32, I64):
            with pytest.raises(TypeError, match="cannot convert"):
                Field("x", src, out=out)
    for src, out in S.pairs():
        assert Field("x", src, (3,), out=out).out_dtype == (src if out is None else out)


def test_field_normalize_refusals():
    from torchkafka_amd import Field

    for dt, out in ((I32, None), (U8, None), (I32, I64), (I64, I32)):
        with pytest.raises(TypeError, match="normalize needs a float destination"):
            Field("x", dt, out=out, normalize=(0.0, 1.0))
    for n in (2, 5, 7):
        with pytest.raises(ValueError, match="1 or 6 elements"):
            Field("x", F32, (2, 3), normalize=(torch.zeros(n), torch.ones(n)))
    with pytest.raises(ValueError, match="1 or 6 elements"):
        Field("x", F32, (2, 3), normalize=(0.0, torch.ones(4)))
    # a float field with out=None is normalised in its own dtype, through the conversion path
    f = Field("x", F16, (2, 3), normalize=(torch.zeros(6), 2.0))
    assert f.out_dtype == F16 and not f.identity
    assert Field("x", I32, out=F32, normalize=(1.0, 2.0)).out_dtype == F32
    assert Field("x", F16).identity and Field("x", F16, out=F16).identity and not Field("x", F16, out=F32).identity


def test_struct_limits_name_the_limit():
    from torchkafka_amd import Field, Struct

    with pytest.raises(ValueError, match="1 to 32 fields"):
        Struct()
    with pytest.raises(ValueError, match="1 to 32 fields"):
        Struct(*(Field(f"f{i}", I32) for i in range(33)))
    assert Struct(*(Field(f"f{i}", I32) for i in range(32))).size == 128
    with pytest.raises(ValueError, match="unique"):
        Struct(Field("a", I32), Field("a", F32))
    with pytest.raises(ValueError, match="non-empty"):
        Field("", I32)
    for shape in ((0,), (2, 0), (-1,)):
        with pytest.raises(ValueError, match="dimension must be >= 1"):
            Field("a", I32, shape)
    with pytest.raises(ValueError, match="below the end of a field"):
        Struct(Field("a", I32, (4,)), size=12)
    with pytest.raises(ValueError, match="below the end of a field"):
        Struct(Field("a", I64, offset=8), Field("b", U8, offset=0), size=12)
    with pytest.raises(ValueError, match="multiple of 4"):
        Struct(Field("a", U8, (7,)))
    with pytest.raises(ValueError, match="multiple of 4"):
        Struct(Field("a", I32), size=6)
    assert Struct(Field("a", U8, (7,)), size=8).size == 8
    with pytest.raises(ValueError, match="32768"):
        Struct(Field("a", F32, (8193,)))
    assert Struct(Field("a", F32, (8192,))).size == 32768
    with pytest.raises(TypeError, match="Field"):
        Struct(("a", I32))


def test_struct_plus_key_is_refused():
    from torchkafka_amd import Key, Timestamp

    for extra in (Key(), Timestamp()):
        with pytest.raises(TypeError, match="carries its label as a field"):
            _ = S.struct52() + extra


# ----------------------------------------------------------------------------- the oracle itself
def test_the_oracle_on_a_hand_packed_record():
    from torchkafka_amd import Field, Struct

    s = Struct(Field("u", U8), Field("f", F32, (2,), out=F16, normalize=(1.0, 4.0)), Field("q", I64, out=I32),
               Field("h", F16, out=F32), size=24)
    assert s.offsets == (0, 1, 9, 17)
    value = (S.le("B", 200) + S.le("2f", 3.0, -7.0) + S.le("q", (5 << 32) + 9) + S.le("e", 1.5)).ljust(24, b"\xee")
    got = S.oracle_record(value, s)
    assert got["u"].item() == 200 and got["u"].dtype == U8
    assert got["f"].tolist() == [0.5, -2.0] and got["f"].dtype == F16
    assert got["q"].item() == 9 and got["q"].dtype == I32           # int64 -> int32 wraps
    assert got["h"].item() == 1.5 and got["h"].dtype == F32
    whole = S.oracle(torch.frombuffer(bytearray(value * 3), dtype=U8).view(3, 24), s)
    assert whole["f"].shape == (3, 2) and whole["u"].shape == (3,) and whole["q"].tolist() == [9, 9, 9]


def test_the_record_generator_places_the_specials():
    s = S.struct52()
    raw = S.random_records(s, 64, 3)
    want = S.oracle(raw, s)
    for name in ("f", "b", "h"):
        v = want[name].to(F32).flatten()
        assert v.isnan().any() and v.isinf().any() and (v == 0).any() and v.isfinite().sum() > v.numel() // 2


# ----------------------------------------------------------------------------- process / reference_struct
@pytest.mark.parametrize("normalize", [None, "scalar", "vector"])
def test_reference_struct_and_process_match_the_oracle_on_every_pair(normalize):
    from torchkafka_amd import reference_struct, split_struct

    for s in S.all_pairs_struct(normalize):
        raw = S.random_records(s, 40, 11)
        want = S.oracle(raw, s)
        S.assert_struct_equal(s, reference_struct(raw, s), want, "uint8 rows")
        S.assert_struct_equal(s, reference_struct(raw.view(I32), s), want, "int32 carrier")
        S.assert_struct_equal(s, split_struct(raw, s), want, "split_struct on the CPU")
        for r in (0, 7, 39):
            rec = SimpleNamespace(value=bytes(raw[r].tolist()), offset=r)
            got = s.process(rec)
            S.assert_struct_equal(s, got, {k: v[r] for k, v in want.items()}, f"process row {r}")


def test_reference_struct_shapes_overlaps_and_one_row():
    from torchkafka_amd import Field, Struct, reference_struct

    s = readme_struct()
    raw = S.random_records(s, 9, 1)
    got = reference_struct(raw, s)
    assert {k: tuple(v.shape) for k, v in got.items()} == {"flag": (9,), "features": (9, 64), "ids": (9, 2, 4),
                                                           "weight": (9,), "label": (9,)}
    S.assert_struct_equal(s, got, S.oracle(raw, s))
    S.assert_struct_equal(s, reference_struct(raw[:1], s), S.oracle(raw[:1], s), "one row")
    empty = reference_struct(raw[:0], s)
    assert {k: tuple(v.shape) for k, v in empty.items()} == {"flag": (0,), "features": (0, 64), "ids": (0, 2, 4),
                                                             "weight": (0,), "label": (0,)}
    assert empty["features"].dtype == BF16
    u = Struct(Field("wide", I64), Field("lo", I32, offset=0), Field("hi", I32, offset=4),
               Field("by", U8, (8,), offset=0))
    raw = S.random_records(u, 5, 2)
    got = reference_struct(raw, u)
    S.assert_struct_equal(u, got, S.oracle(raw, u))
    assert torch.equal((got["hi"].long() << 32) | (got["lo"].long() & 0xFFFFFFFF), got["wide"])


def test_split_struct_argument_errors():
    from torchkafka_amd import split_struct

    s = S.struct52()
    for bad in (torch.zeros(4, 52, dtype=I8), torch.zeros(4, 12, dtype=I32), torch.zeros(4, 51, dtype=U8),
                torch.zeros(52, dtype=U8), torch.zeros(4, 13, dtype=F32)):
        with pytest.raises(ValueError, match=r"int32 \[rows, 13\] or uint8 \[rows, 52\]"):
            split_struct(bad, s)
    with pytest.raises(ValueError, match="contiguous"):
        split_struct(torch.zeros(4, 104, dtype=U8)[:, ::2], s)


def test_process_treats_a_wrong_size_as_fixed_width_does():
    s, lax = S.struct52(), S.struct52(skip_bad=True)
    assert s.process(SimpleNamespace(value=None, offset=0)) is None
    for n in (51, 53, 0):
        with pytest.raises(ValueError, match=f"value size {n} != 52"):
            s.process(SimpleNamespace(value=b"x" * n, offset=3))
        assert lax.process(SimpleNamespace(value=b"x" * n, offset=3)) is None


# ----------------------------------------------------------------------------- the CPU loader
PARTS, PER_PART, BS = S.PARTS, S.PER_PART, S.BS
produce_struct, check_batches = S.produce_struct, S.check_batches


def test_cpu_loader_end_to_end_with_exact_commits(broker):
    from torchkafka_amd import auto_commit

    s = S.struct52()
    rows = produce_struct(broker, s)
    dl = _loader(broker, _dataset(s), BS, "cpu", "g")
    batches = list(auto_commit(dl))
    dl.close()
    check_batches(s, rows, batches, "cpu")
    assert sum(b["u"].shape[0] for b in batches) == PARTS * PER_PART
    assert min(b["u"].shape[0] for b in batches) < BS  # a partial batch was delivered
    assert broker.committed_offsets("g", "t") == {0: 70, 1: 70, 2: 70}


def test_cpu_loader_return_info_carries_the_dict(broker):
    from torchkafka_amd import KafkaBatch, auto_commit

    s = S.struct52()
    rows = produce_struct(broker, s, seed=1)
    dl = _loader(broker, _dataset(s), BS, "cpu", "g", return_info=True)
    items = list(auto_commit(dl))
    dl.close()
    assert all(isinstance(i, KafkaBatch) and i.lengths is None and i.mask is None for i in items)
    assert sum(i.n_records for i in items) == PARTS * PER_PART
    check_batches(s, rows, [i.data for i in items], "cpu")
    assert broker.committed_offsets("g", "t") == {0: 70, 1: 70, 2: 70}


def test_cpu_loader_skip_bad_skips_a_wrong_size_record_and_commits_it(broker):
    from torchkafka_amd import auto_commit

    lax = S.struct52(skip_bad=True)
    rows = produce_struct(broker, lax, seed=2, bad_at=(1, 17))
    dl = _loader(broker, _dataset(lax), BS, "cpu", "lax")
    batches = list(auto_commit(dl))
    dl.close()
    check_batches(lax, rows, batches, "cpu")
    assert broker.committed_offsets("lax", "t") == {0: 70, 1: 71, 2: 70}
    strict = _loader(broker, _dataset(S.struct52()), BS, "cpu", "strict")
    with pytest.raises(Exception, match="value size does not match the fixed-width schema"):  # FixedWidth's refusal
        list(auto_commit(strict))
    strict.close()


def test_torch_dataloader_compat_path_gives_the_same_dicts(broker):
    from torch.utils.data import DataLoader

    from torchkafka_amd import auto_commit

    s = readme_struct()
    broker.create_topic("t", 1)
    raw = S.random_records(s, 50, 9)
    broker.produce("t", [bytes(r.tolist()) for r in raw], partition=0)
    DS = _dataset(s)
    ds = DS("t", bootstrap_servers=broker.url, group_id="ref", auto_offset_reset="earliest", consumer_timeout_ms=250)
    ref = list(DataLoader(ds, batch_size=16))
    dl = _loader(broker, DS, 16, "cpu", "dl")
    got = list(auto_commit(dl))
    dl.close()
    assert len(ref) == len(got) == 4
    want = S.oracle(raw, s)
    for k, (a, b) in enumerate(zip(ref, got)):
        S.assert_struct_equal(s, a, {n: v[16 * k:16 * k + 16] for n, v in want.items()}, f"DataLoader batch {k}")
        S.assert_struct_equal(s, b, a, f"DeviceLoader batch {k}")


def test_a_process_override_keeps_the_per_record_path(broker):
    """A dataset that maps records itself is not split: its samples are whatever it returns."""
    from torchkafka_amd import KafkaDataset, auto_commit

    s = S.struct52()

    class Own(KafkaDataset):
        schema = s

        def _process(self, record):
            return torch.frombuffer(bytearray(record.value), dtype=U8).clone()

    rows = produce_struct(broker, s, seed=4)
    dl = _loader(broker, Own, BS, "cpu", "own")
    got = torch.cat(list(auto_commit(dl)))
    dl.close()
    assert got.dtype == U8 and got.shape == (PARTS * PER_PART, 52)
    stamps = got[:, 35:39].contiguous().view(I32).flatten()
    assert torch.equal(got[torch.argsort(stamps)], torch.cat(rows))


# ----------------------------------------------------------------------------- loader options
def _construct(schema, **kw):
    from torchkafka_amd import DeviceLoader

    DS = _dataset(schema)
    return DeviceLoader(DS.placeholder(), 4, num_workers=1, device="cpu",
                        worker_init_fn=DS.init_worker("t", bootstrap_servers="shm://nowhere", group_id="g"), **kw)


def test_loader_option_refusals():
    s = S.struct52()
    for kw in ({"dtype": BF16}, {"dtype": I32}, {"normalize": (0.0, 1.0)}):
        with pytest.raises(TypeError, match="on its fields"):
            _construct(s, **kw)
    for q in ("mxfp8", "mxfp4"):
        with pytest.raises(TypeError, match="quantize"):
            _construct(s, quantize=q)
    for kw in ({"layout": "packed"}, {"layout": "binned", "seq_len": 64}):
        with pytest.raises(TypeError, match="layout"):
            _construct(s, **kw)
    dl = _construct(s)
    assert dl.plan.kind == 0 and dl._n_extras() == 0


def test_other_schemas_keep_their_native_stages():
    """With any other schema the struct stage returns the callable it was given."""
    from torchkafka_amd import FixedWidth

    dl = _construct(FixedWidth(F32, (8,)))
    marker = object()
    assert dl._struct is None and dl._struct_stage(marker) is marker


# ----------------------------------------------------------------------------- the example
def test_example_09_runs_on_the_cpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "09_struct_records.py"), "--device", "cpu",
                        "--records", "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 struct records on cpu, 0 field mismatches" in r.stdout
    assert "{0: 150, 1: 150}" in r.stdout
