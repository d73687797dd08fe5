"""An independent oracle and input builder for the span kernels (span_decode.hip, span_device.h).

Nothing here calls the package: the CRC32C is a 256-entry table built in this file from the
polynomial, the "log" is a plain byte string.  The kernels do not parse Kafka framing -- they are
handed byte ranges (segments), row positions and flags -- so neither does this builder.

* ``crc32c_raw``      the reflected CRC32C register after ``data`` (no final xor), from ``init``;
* ``crc32c``          the standard checksum (init and final xor 0xFFFFFFFF);
* ``segment_raw``     what a segment's workgroup must leave in ``partials``;
* ``sweep_cases``     the (length, first, last) table the CPU and GPU CRC sweeps share;
* ``LogBuilder``      random framing bytes with payloads placed at chosen ``address & 15``.
"""
import random

POLY = 0x82F63B78  # CRC32C (Castagnoli), reflected
FRONT = 21         # bytes of a RecordBatch before its CRC'd range (base offset .. the CRC field)
SLACK = 64         # bytes kept on both sides of every placed payload


def make_table(poly: int = POLY):
    t = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ (poly if c & 1 else 0)
        t.append(c)
    return t


TABLE = make_table()


def crc32c_raw(data, init: int = 0, table=None) -> int:
    """The CRC32C register after ``data``, starting from ``init``; no final xor."""
    t = TABLE if table is None else table
    c = init & 0xFFFFFFFF
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c


def crc32c(data, table=None) -> int:
    return crc32c_raw(data, 0xFFFFFFFF, table) ^ 0xFFFFFFFF


def raw_bitwise(data, init: int = 0) -> int:
    """The register again, bit by bit and without a table (the table's own check)."""
    c = init & 0xFFFFFFFF
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c


def crc32c_bitwise(data) -> int:
    return raw_bitwise(data, 0xFFFFFFFF) ^ 0xFFFFFFFF


def segment_raw(data, first: bool) -> int:
    """The raw CRC a workgroup owes for the segment ``data``: the segment holding a RecordBatch's
    start skips its first 21 bytes and starts from 0xFFFFFFFF, every other one starts from zero."""
    return crc32c_raw(bytes(data)[FRONT:], 0xFFFFFFFF) if first else crc32c_raw(data, 0)


def chain(parts):
    """``parts``: (raw CRC, CRC'd bytes) per consecutive segment of one RecordBatch -> its checksum.
    Moving a register over n bytes of the next segment is n zero bytes fed from it (CRC linearity)."""
    acc = 0
    for raw, n in parts:
        acc = crc32c_raw(bytes(n), acc) ^ raw
    return acc ^ 0xFFFFFFFF


def sweep_lengths(W: int, seg_max: int):
    tiny = [1, 3, 4, 5, 19, 20, 21]
    rest = [61, 62, 81, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 21, 3 * W + 7, 4 * W, seg_max - 1, seg_max]
    return tiny, rest


def sweep_cases(W: int, seg_max: int):
    """(length, first, last) of the CRC value sweep: middle and last pieces at every length, first
    pieces from 61 bytes (a first segment is never shorter than the RecordBatch header)."""
    tiny, rest = sweep_lengths(W, seg_max)
    cases = []
    for n in tiny + rest:
        cases.append((n, False, False))
        cases.append((n, False, True))
    for n in rest:
        cases.append((n, True, False))
    return cases


_DATA = {}


def sweep_data(n: int, seed: int = 0) -> bytes:
    """The sweep's bytes for a length (cached: the CPU and GPU tests feed the same bytes)."""
    key = (n, seed)
    if key not in _DATA:
        _DATA[key] = random.Random(1_000_003 * seed + n).randbytes(n)
    return _DATA[key]


_RAW = {}


def sweep_raw(n: int, first: bool, seed: int = 0) -> int:
    key = (n, first, seed)
    if key not in _RAW:
        _RAW[key] = segment_raw(sweep_data(n, seed), first)
    return _RAW[key]


class LogBuilder:
    """A byte string of random framing bytes with payloads at chosen positions.

    Byte 0 of the string is meant to sit at a 16-byte aligned address (``upload``), so a payload
    placed with ``align=a`` has ``address & 15 == a``.  Every payload has at least ``SLACK`` random
    bytes before it and the string ends with ``SLACK`` more: the loader wave stages whole 16-byte
    chunks and reads up to 15 bytes outside a segment.  Positions are log positions: offsets into
    the string plus ``base`` (past 2^32: positions are 64-bit)."""

    def __init__(self, seed: int, base: int = (5 << 32) + 4096):
        assert base % 16 == 0
        self.rng = random.Random(seed)
        self.base = base
        self.buf = bytearray(self.rng.randbytes(SLACK))

    def pos(self) -> int:
        return self.base + len(self.buf)

    def frame(self, n: int) -> None:
        """``n`` random framing bytes."""
        self.buf += self.rng.randbytes(n)

    def align(self, a: int, gap: int = 0) -> None:
        """Framing bytes (at least ``gap``) so that the next byte sits at ``address & 15 == a``."""
        self.frame(gap)
        self.frame((a - len(self.buf)) & 15)

    def put(self, data) -> int:
        """Appends ``data``; returns its log position."""
        p = self.pos()
        self.buf += bytes(data)
        return p

    def reserve(self, n: int) -> int:
        """``n`` bytes to be filled in later (``write``); returns their log position."""
        return self.put(bytes(n))

    def write(self, pos: int, data) -> None:
        data = bytes(data)
        o = pos - self.base
        assert 0 <= o and o + len(data) <= len(self.buf)
        self.buf[o:o + len(data)] = data

    def place(self, data, align: int) -> int:
        """``data`` at ``address & 15 == align`` with ``SLACK`` framing bytes before it."""
        self.align(align, SLACK)
        return self.put(data)

    def bytes_at(self, pos: int, n: int) -> bytes:
        return bytes(self.buf[pos - self.base:pos - self.base + n])

    def finish(self) -> bytes:
        self.frame(SLACK)
        return bytes(self.buf)

    def upload(self):
        """-> (device uint8 tensor to keep alive, address of log position ``base``)."""
        import torch

        raw = self.finish()
        t = torch.empty(len(raw) + 16, dtype=torch.uint8, device="cuda")
        off = (-t.data_ptr()) & 15
        t[off:off + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        return t, t.data_ptr() + off
