"""Declarative record schemas: the native fast path's contract with a dataset.

The reference has one way to turn a record into a sample: a Python
``_process(record)`` per record (kafka_dataset.py:173-186).  A dataset that
declares ``schema = FixedWidth(...)``, ``VarLen(...)`` or ``JsonArray(...)``
additionally lets :class:`~torchkafka_amd.loader.DeviceLoader` decode whole
batches natively (C++ packer into the pinned ring, gfx950 collate kernel on
device) while keeping the per-record semantics, including the reference's
``None``-skip: a null value, or a row shorter than ``min_len``, is skipped and
still advances (and is committed with) the partition position (B6).

Every schema also provides ``process(record)``: the exact per-record
equivalent used by the torch-DataLoader compat path, so one dataset class
works with both loaders and both produce identical samples.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass

import torch

from ..ops.native import core

_DT_CODE = {
    torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float8_e4m3fn: 3, torch.uint8: 4,
    torch.int8: 5, torch.int32: 6, torch.int64: 7,
}


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT_CODE[dt]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}") from None


@dataclass(frozen=True)
class FixedWidth:
    """Each record value is ``prod(shape)`` raw little-endian elements of ``dtype``."""

    dtype: torch.dtype = torch.float32
    shape: tuple = (256,)
    skip_bad: bool = False

    kind = 0

    @property
    def row_elems(self) -> int:
        return int(math.prod(self.shape))

    @property
    def elem_size(self) -> int:
        return torch.empty((), dtype=self.dtype).element_size()

    @property
    def row_bytes(self) -> int:
        return self.row_elems * self.elem_size

    def process(self, record):
        v = record.value
        if v is None:
            return None
        if len(v) != self.row_bytes:
            if self.skip_bad:
                return None
            raise ValueError(f"record at offset {record.offset}: value size {len(v)} != {self.row_bytes}")
        return torch.frombuffer(bytearray(v), dtype=self.dtype).view(self.shape)

    def native_spec(self) -> tuple:
        return (core().PACK_FIXED, self.elem_size, self.row_elems, 0, -1, True, self.skip_bad)

    def __add__(self, field):
        return WithFields(self, (field,))

    # record fields beside the value (see WithFields): none
    fields: tuple = ()


@dataclass(frozen=True)
class VarLen:
    """Each record value is a variable number of raw ``dtype`` elements (e.g. int32 token ids)."""

    dtype: torch.dtype = torch.int32
    min_len: int = 0
    max_len: int | None = None
    truncate: bool = True
    skip_bad: bool = False

    kind = 1

    @property
    def elem_size(self) -> int:
        return torch.empty((), dtype=self.dtype).element_size()

    def _filter(self, t):
        n = t.numel()
        if n < self.min_len:
            return None
        if self.max_len is not None and n > self.max_len:
            if not self.truncate:
                return None
            t = t[: self.max_len]
        return t

    def process(self, record):
        v = record.value
        if v is None:
            return None
        if len(v) % self.elem_size:
            if self.skip_bad:
                return None
            raise ValueError(f"record at offset {record.offset}: size not a multiple of {self.elem_size}")
        return self._filter(torch.frombuffer(bytearray(v), dtype=self.dtype) if v else
                            torch.empty(0, dtype=self.dtype))

    def native_spec(self) -> tuple:
        return (core().PACK_VARLEN, self.elem_size, 0, self.min_len,
                -1 if self.max_len is None else self.max_len, self.truncate, self.skip_bad)


@dataclass(frozen=True)
class JsonArray(VarLen):
    """Each record value is a flat JSON array of numbers, decoded to float32 (README.md:54,74 pattern)."""

    dtype: torch.dtype = torch.float32

    kind = 2

    @property
    def elem_size(self) -> int:
        return 4

    def process(self, record):
        v = record.value
        if v is None:
            return None
        try:
            vals = json.loads(v)
            if not isinstance(vals, list) or any(isinstance(x, (list, dict, str, bool)) or x is None for x in vals):
                raise ValueError
            t = torch.tensor([float(x) for x in vals], dtype=torch.float32)
        except ValueError:
            if self.skip_bad:
                return None
            raise ValueError(f"record at offset {record.offset}: not a flat numeric JSON array") from None
        return self._filter(t)

    def native_spec(self) -> tuple:
        return (core().PACK_JSON_F32, 4, 0, self.min_len, -1 if self.max_len is None else self.max_len,
                self.truncate, self.skip_bad)


# ---------------------------------------------------------------- record fields beside the value

_KEY_ENCODINGS = {"be": 0, "le": 1, "ascii": 2}


@dataclass(frozen=True)
class Key:
    """The record key as an int64 label beside the value: ``encoding`` "be" (8 bytes big-endian,
    Kafka's LongSerializer -- the default), "le" (8 bytes little-endian) or "ascii" (decimal
    digits).  A null key, or one the encoding cannot read, gives ``default``."""

    encoding: str = "be"
    default: int = -1

    bit = 1  # csrc/core/consumer.h kExtraKey

    def __post_init__(self):
        if self.encoding not in _KEY_ENCODINGS:
            raise ValueError(f"Key encoding {self.encoding!r}: one of {sorted(_KEY_ENCODINGS)}")

    def value_of(self, record) -> int:
        return int(core().key_int64(record.key, _KEY_ENCODINGS[self.encoding], int(self.default)))


@dataclass(frozen=True)
class Timestamp:
    """The record timestamp (ms, int64) beside the value."""

    bit = 2  # csrc/core/consumer.h kExtraTimestamp

    def value_of(self, record) -> int:
        return int(record.timestamp)


@dataclass(frozen=True)
class WithFields:
    """A fixed-width value plus per-record fields, e.g. ``FixedWidth(torch.float32, (256,)) +
    Key()`` -- a label riding with the features (the reference README's ``(features, label)``
    samples, README.md:40-44).  Batches are ``(values, key, timestamp)`` in the order the fields
    were added, each field an int64 tensor of one element per row.  On the device path the worker
    reads the fields while it walks the record headers and the gfx950 decode kernel copies them
    into the batch beside the values (no extra launch)."""

    value: FixedWidth
    fields: tuple = ()

    def __post_init__(self):
        if not isinstance(self.value, FixedWidth):
            raise TypeError("record fields ride with a FixedWidth value schema")
        bits = [f.bit for f in self.fields]
        if len(set(bits)) != len(bits):
            raise ValueError("each record field can be added once")
        if any(not isinstance(f, (Key, Timestamp)) for f in self.fields):
            raise TypeError("fields: Key() and/or Timestamp()")

    def __add__(self, field):
        return WithFields(self.value, self.fields + (field,))

    # the value schema's interface
    kind = 0

    @property
    def dtype(self):
        return self.value.dtype

    @property
    def shape(self):
        return self.value.shape

    @property
    def skip_bad(self):
        return self.value.skip_bad

    @property
    def row_elems(self) -> int:
        return self.value.row_elems

    @property
    def elem_size(self) -> int:
        return self.value.elem_size

    @property
    def row_bytes(self) -> int:
        return self.value.row_bytes

    def native_spec(self) -> tuple:
        return self.value.native_spec()

    def extras_spec(self) -> tuple:
        """(field bits, key encoding, key default) for the native packer; the columns are stored
        key first, then timestamp -- :meth:`column_order` maps them back to the order added."""
        key = next((f for f in self.fields if isinstance(f, Key)), None)
        bits = 0
        for f in self.fields:
            bits |= f.bit
        return bits, _KEY_ENCODINGS[key.encoding] if key else 0, int(key.default) if key else -1

    def column_order(self) -> list[int]:
        """Index of each added field among the native columns (key, timestamp)."""
        native = sorted(self.fields, key=lambda f: f.bit)
        return [native.index(f) for f in self.fields]

    def process(self, record):
        v = self.value.process(record)
        if v is None:
            return None
        return (v, *(torch.tensor(f.value_of(record), dtype=torch.int64) for f in self.fields))


# ---------------------------------------------------------------- multi-field records

_FIELD_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int32, torch.int64)
_FIELD_OUT = (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.int32, torch.int64)
_FLOAT_OUT = (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn)
STRUCT_MAX_FIELDS = 32      # csrc/hip/collate.h kStructMaxFields
STRUCT_MAX_SIZE = 32768     # csrc/hip/collate.h kStructMaxRecord
STRUCT_COPY = -1            # csrc/hip/collate.h kStructCopy: the field's bytes, unchanged


class Field:
    """One member of a :class:`Struct`: ``prod(shape)`` little-endian elements of ``dtype`` at byte
    ``offset`` of the record value (default: the end of the field declared before it -- packed, no
    implicit alignment).  Delivered as ``[rows, *shape]`` (``shape=()``: ``[rows]``).

    ``out=None`` copies the field's bytes unchanged in its own dtype (NaN payloads kept); otherwise
    the field is converted to ``out`` exactly as ``Tensor.to`` converts.  ``normalize=(mean, std)``
    (1 or ``prod(shape)`` elements each) needs a float destination -- ``out``, or the field's own
    dtype when ``out`` is None -- and delivers ``(float32(x) - mean) * (1 / std)`` computed in
    float32 and rounded once to the destination."""

    def __init__(self, name: str, dtype: torch.dtype, shape=(), *, out: torch.dtype | None = None, normalize=None,
                 offset: int | None = None):
        if not isinstance(name, str) or not name:
            raise ValueError("Field: the name must be a non-empty string")
        if dtype not in _FIELD_DTYPES:
            raise TypeError(f"Field {name!r}: dtype must be one of float32, float16, bfloat16, uint8, int8, int32, "
                            f"int64, not {dtype}")
        if out is not None and out not in _FIELD_OUT:
            raise TypeError(f"Field {name!r}: out must be None or one of float32, float16, bfloat16, float8_e4m3fn, "
                            f"int32, int64, not {out}")
        if out is not None and dtype.is_floating_point and out not in _FLOAT_OUT:
            raise TypeError(f"Field {name!r}: cannot convert {dtype} records to {out}")
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(d) for d in shape)
        if any(d < 1 for d in shape):
            raise ValueError(f"Field {name!r}: every shape dimension must be >= 1, got {shape}")
        if offset is not None and int(offset) < 0:
            raise ValueError(f"Field {name!r}: offset must be >= 0")
        self.name, self.dtype, self.shape, self.out = name, dtype, shape, out
        self.offset = None if offset is None else int(offset)
        self.elems = int(math.prod(shape))
        self.elem_size = torch.empty((), dtype=dtype).element_size()
        self.nbytes = self.elems * self.elem_size
        self.out_dtype = dtype if out is None else out
        self.normalize = normalize
        self.shift = self.scale = None  # CPU f32 [elems]: (x - shift) * scale
        self._on_device: dict = {}      # device -> (shift, scale) there, made once
        if normalize is not None:
            if self.out_dtype not in _FLOAT_OUT:
                raise TypeError(f"Field {name!r}: normalize needs a float destination, not {self.out_dtype} (set out=)")
            from ..ops.collate import normalize_params

            try:
                self.shift, self.scale = normalize_params(normalize, self.elems, "cpu")
            except ValueError:
                raise ValueError(f"Field {name!r}: normalize mean/std must have 1 or {self.elems} elements") from None
        # copied unchanged: no out (or the field's own dtype) and nothing to compute
        self.identity = normalize is None and self.out_dtype == dtype

    def __repr__(self):
        extra = "".join(f", {k}={v}" for k, v in (("out", self.out), ("offset", self.offset)) if v is not None)
        return (f"Field({self.name!r}, {self.dtype}, {self.shape}{extra}"
                f"{', normalize=...' if self.normalize is not None else ''})")

    def convert(self, x: torch.Tensor) -> torch.Tensor:
        """``x`` (this field's dtype, ``[..., *shape]``, any device) as it is delivered."""
        if self.identity:
            return x
        if self.out_dtype not in _FLOAT_OUT:
            return x.to(self.out_dtype)
        y = x.to(torch.float32)
        if self.shift is not None:
            shift, scale = self.affine_on(x.device)
            y = (y - shift.view(self.shape)) * scale.view(self.shape)
        return y.to(self.out_dtype)

    def affine_on(self, device):
        """(shift, scale) as f32 [elems] vectors on ``device`` (kept here: the kernel's field table
        holds their addresses), or None without ``normalize``."""
        if self.shift is None:
            return None
        device = torch.device(device)
        got = self._on_device.get(device)
        if got is None:
            got = self._on_device[device] = (self.shift.to(device), self.scale.to(device))
        return got

    def __getstate__(self):  # device tensors stay behind when a dataset travels to a spawned worker
        state = dict(self.__dict__)
        state["_on_device"] = {}
        return state


class Struct:
    """Each record value is a little-endian packed struct of ``size`` bytes; a batch is a dict
    ``{field name: tensor [rows, *shape]}``.

    The record travels through the loader as a fixed-width int32 carrier,
    ``FixedWidth(torch.int32, (size // 4,))``: workers, the ring and the decode kernels see that
    schema (this class exposes its interface), and one gfx950 launch behind the decode
    (csrc/hip/struct_split.hip, :func:`torchkafka_amd.ops.collate.split_struct`) splits the delivered
    ``[rows, size / 4]`` batch into the per-field tensors, converting and normalising on the way.

    Fields may leave gaps and may overlap (a union read two ways).  ``size`` defaults to the end of
    the last declared field; it must be a multiple of 4 (the carrier is int32 words: a producer
    rounds an odd struct up) and at most 32768.  A value of another size is treated as
    ``FixedWidth`` treats it (``skip_bad``)."""

    kind = 0
    fields: tuple = ()  # record fields beside the value (WithFields): none -- the label lives in the struct

    def __init__(self, *members: Field, size: int | None = None, skip_bad: bool = False):
        if not 1 <= len(members) <= STRUCT_MAX_FIELDS:
            raise ValueError(f"Struct: 1 to {STRUCT_MAX_FIELDS} fields, got {len(members)}")
        if any(not isinstance(f, Field) for f in members):
            raise TypeError("Struct: the members are Field(...) objects")
        names = [f.name for f in members]
        if len(set(names)) != len(names):
            raise ValueError(f"Struct: field names must be unique, got {names}")
        offsets, end, last_end = [], 0, 0
        for f in members:
            off = end if f.offset is None else f.offset
            offsets.append(off)
            end = off + f.nbytes
            last_end = max(last_end, end)
        size = end if size is None else int(size)
        if size < last_end:
            raise ValueError(f"Struct: size={size} is below the end of a field ({last_end})")
        if size % 4:
            raise ValueError(f"Struct: size={size} must be a multiple of 4 (the record travels as int32 words; "
                             "round size= up, the producer pads the record)")
        if size > STRUCT_MAX_SIZE:
            raise ValueError(f"Struct: size={size} is above {STRUCT_MAX_SIZE} bytes (a bigger record is a tensor: "
                             "use FixedWidth)")
        self.members = tuple(members)
        self.offsets = tuple(offsets)
        self.size = size
        self.carrier = FixedWidth(torch.int32, (size // 4,), bool(skip_bad))
        self._device_specs: dict = {}

    def __repr__(self):
        return f"Struct({', '.join(map(repr, self.members))}, size={self.size})"

    def __add__(self, field):
        raise TypeError("Struct + Key() / Timestamp() is not supported: a struct record carries its label as a field")

    # the value-schema interface: the carrier's
    @property
    def dtype(self):
        return self.carrier.dtype

    @property
    def shape(self):
        return self.carrier.shape

    @property
    def skip_bad(self):
        return self.carrier.skip_bad

    @property
    def row_elems(self) -> int:
        return self.carrier.row_elems

    @property
    def elem_size(self) -> int:
        return self.carrier.elem_size

    @property
    def row_bytes(self) -> int:
        return self.carrier.row_bytes

    def native_spec(self) -> tuple:
        return self.carrier.native_spec()

    def device_spec(self, device) -> list:
        """The field table ``hip().struct_tensors`` takes: per field (offset, shape, source dtype
        code, destination dtype code or STRUCT_COPY, shift address, scale address), the shift / scale
        vectors on ``device`` (made once per device, kept alive by the fields)."""
        device = torch.device(device)
        spec = self._device_specs.get(device)
        if spec is None:
            spec = []
            for f, off in zip(self.members, self.offsets):
                aff = f.affine_on(device)
                shift, scale = (aff[0].data_ptr(), aff[1].data_ptr()) if aff is not None else (0, 0)
                spec.append((off, f.shape, _DT_CODE[f.dtype], STRUCT_COPY if f.identity else _DT_CODE[f.out_dtype],
                             shift, scale))
            self._device_specs[device] = spec
        return spec

    def __getstate__(self):  # device tensors stay behind when a dataset travels to a spawned worker
        state = dict(self.__dict__)
        state["_device_specs"] = {}
        return state

    def process(self, record):
        v = record.value
        if v is None:
            return None
        if len(v) != self.size:
            if self.skip_bad:
                return None
            raise ValueError(f"record at offset {record.offset}: value size {len(v)} != {self.size}")
        out = {}
        for f, off in zip(self.members, self.offsets):
            x = torch.frombuffer(bytearray(v[off:off + f.nbytes]), dtype=f.dtype).view(f.shape)
            out[f.name] = f.convert(x)
        return out
