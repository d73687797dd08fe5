"""DeviceLoader: Kafka records -> collated device tensors with exact per-batch commits.

Data path per batch (MI355X-first, no torch DataLoader on the hot path):

  worker process                         main process                       GPU
  ----------------------------------    ---------------------------------  -----------------------------
  fetch RecordBatches from the broker
  log, CRC-check, None-skip filter,
  pack values into a pinned ring slot
  (native C++; or `_process` + stack)
  publish slot (futex)          ----->  acquire READY slot
                                        hipMemcpyAsync slot -> staging      copy stream (side stream)
                                        (issued `prefetch` batches ahead,
                                         so the copy of k+1 overlaps the
                                         user's step k)
                                        stream-wait(h2d event)               compute stream:
                                        collate kernel launch        ----->  stack/pad + cast bf16/fp8
                                                                             (+ fused normalisation)
                                        slot FREE once its DMA is done
                                        yield device tensor
  ...                                   next(): commit batch k's offset
                                        watermarks to the broker (exact),
                                        lock-stepped over RCCL when DDP

Every slot carries the exact per-partition offsets of the records packed in
it, so commits cover exactly what the user has finished (reference D3),
whatever the prefetch depth and whichever worker produced the batch (D5).
"""
from __future__ import annotations

import ctypes
import logging
import time
from typing import NamedTuple

import torch

from ..client.errors import CorruptRecordException
from ..config import LoaderConfig
from ..models.schema import Struct
from ..ops.collate import (CODE_DTYPE, DTYPE_CODE, FLOAT_DTYPES, MX_BLOCK, MX_FORMATS, BinnedBatch, MXBatch,
                           PackedBatch, _stream_ptr, bin_launch, mx_launch, normalize_params, pack_launch, pad_bits,
                           reference_binned, reference_mx, reference_packed, reference_struct, split_struct,
                           struct_launch)
from ..ops.native import core, hip
from ..parallel.sharding import dist_rank_world
from ..utils.metrics import LoaderStats
from ..utils.tracing import enabled as _roctx_enabled
from ..utils.tracing import trace_range
from .bridging import LoaderBridges
from .commits import LoaderCommits
from .lockstep import LoaderLockstep, _host_allreduce_min
from .path_plan import PathPlan
from .run import WorkerError, _Run

log = logging.getLogger(__name__)
_ds_logger = logging.getLogger("torchkafka.kafka_dataset")


def _traced_step(step):
    """A native iteration step inside one roctx range (``TORCHKAFKA_ROCTX=1``)."""
    def traced():
        with trace_range("torchkafka.next_batch"):
            return step()
    return traced


class KafkaBatch(NamedTuple):
    """Batch plus provenance (``return_info=True``)."""

    data: torch.Tensor    # layout="packed" / "binned": a PackedBatch / BinnedBatch (lengths and mask are then None);
                          # quantize="mxfp8" / "mxfp4": an MXBatch; a Struct schema: the dict of field tensors
    lengths: torch.Tensor | None
    mask: torch.Tensor | None
    watermarks: list      # [(pidx, first_offset, next_offset, n_records)]
    n_records: int        # records consumed incl. skipped ones


class DeviceLoader(LoaderBridges, LoaderCommits, LoaderLockstep):
    """Streams a :class:`KafkaDataset` to device tensors.

    Mirrors ``DataLoader(dataset, batch_size, num_workers, worker_init_fn)``
    (reference README.md:109-127) and adds the device path.  Iterate it
    directly (no commits; call :meth:`commit`) or through
    :func:`~torchkafka_amd.auto_commit` (commit after every batch).

    Args:
        dataset: a ``KafkaDataset`` placeholder (workers build consumers via ``worker_init_fn``), or
            -- with ``num_workers=0`` -- a dataset built with its consumer (``YourDataset(topic, ...)``).
        batch_size: records per batch (per rank).
        num_workers: consumer/packer processes; 0 = the reference's single-process mode
            (auto_commit.py:49-58): a thread of this process consumes and packs the pinned ring
            slots with the dataset's own consumer, and the device path is unchanged.
        worker_init_fn: usually ``YourDataset.init_worker(topic, group_id=..., bootstrap_servers=...)``.
        device: target device (default: current CUDA device, else CPU).
        dtype: output dtype (default: the schema's); floats may go to bf16/f16/fp8 (OCP e4m3fn).
        config: a :class:`~torchkafka_amd.config.LoaderConfig` (or its dict form).  Every field below
            can also be passed as a keyword argument, which overrides the config; the performance
            knobs (``slots_per_worker``, ``slot_bytes``, ``prefetch``, ``copy_streams``,
            ``event_every``, ``coalesce``, ``coalesce_wait_us``, ``lockstep_depth``, ``numa_bind``,
            ``ahead_depth``, ``decode_streams``, ``worker_spin_us``, ``json_count``, ...) form its
            :class:`~torchkafka_amd.config.Tuning` (docs/CONFIG.md).  Options:
        normalize: optional ``(mean, std)`` fused into the collate kernel.
        sharding: ``"static"`` rank/worker partition map (default) or ``"group"`` (Kafka group assignment).
        slots_per_worker: ring depth per worker (prefetched batches in pinned memory).  Default: as
            deep as 8 slots while the whole ring stays within 64 MiB of pinned memory (at least 4).
            Slots whose kernels are still queued on the GPU stay held, so a shallow ring starves
            the workers (config 2 on MI355X: 4 slots 29-31 M rec/s, 8 slots 30-33 M).
        prefetch: batches whose H2D copy is issued ahead of the user (overlap with compute).
        in_order: strict worker round-robin (reference order) instead of first-ready.
        pad_to: var-len / JSON batches are padded to this fixed width (use the schema's ``max_len`` /
            ``truncate`` to bound the rows); None pads each batch to its longest row.
        pad_multiple: with ``pad_to=None``, the batch width is rounded up to a multiple of this.
        pad_value: the value written into the padding.
        return_mask: var-len / JSON batches also yield a bool ``[rows, width]`` mask of real elements.
        layout: ``"padded"`` (default: var-len / JSON batches are ``[rows, width]`` + lengths) or ``"packed"``:
            each batch is a :class:`~torchkafka_amd.PackedBatch` -- flat ``values[capacity]`` with the rows back
            to back and the pad value behind them, int32 ``cu_seqlens[rows + 1]``, ``max_seqlen`` (the padded
            width, an upper bound on the longest row; exact with ``pad_to=None, pad_multiple=1``) and a 0-dim
            device ``total`` -- made from the padded batch by one more gfx950 launch (csrc/hip/pack.hip).
            ``pad_to``, ``pad_multiple``, ``pad_value``, ``dtype`` and the schema's ``max_len`` / ``truncate``
            keep their meaning; there is no mask.  Fixed-width and structured schemas raise ``TypeError``.
            ``"binned"``: several rows packed into each fixed-length sequence, see ``seq_len``.
        pack_to: ``layout="packed"``: the capacity of every batch's ``values`` (static shapes with
            ``drop_last=True``, e.g. for graph capture).  Rows beyond it are cut: ``cu_seqlens`` is clamped to it
            and ``total > pack_to`` shows the overflow, without a sync.  None: ``rows * width``, nothing is ever cut.
        return_ids: ``layout="packed"``: also int32 ``position_ids`` / ``segment_ids`` ``[capacity]`` (index inside
            the row / row index; 0 / -1 behind the last row).
        seq_len: ``layout="binned"`` (required there): each batch is a :class:`~torchkafka_amd.BinnedBatch` --
            ``values[bins, seq_len]`` with several rows packed into each fixed-length sequence, first-fit in arrival
            order, int32 ``segment_ids`` / ``position_ids`` of the same shape (row index / index inside the row;
            -1 / 0 in padding), ``bin_lens``, ``row_bin`` / ``row_start`` / ``row_lens`` and the 0-dim device
            ``n_bins`` / ``unplaced`` / ``cut`` -- made from the padded batch by two more gfx950 launches
            (csrc/hip/bin.hip).  A row longer than ``seq_len`` is cut there (``cut`` counts the elements lost).
            The padded-batch options keep their meaning, as for ``"packed"``; there is no mask.
        bins: ``layout="binned"``: the number of sequences of every batch (static shapes with ``drop_last=True``).
            None: one per row, so every row finds a bin.  With fewer, a row that fits no bin is left out
            (``row_bin == -1``, counted in ``unplaced``; later rows may still fit).  Such rows, and cut ones, are
            still committed with their batch -- exactly as ``pack_to`` treats an overflow; nothing is carried over
            into the next batch.  At most 16384 rows and bins per batch on the GPU.
        quantize: ``None`` (default) or ``"mxfp8"`` / ``"mxfp4"``: the batch's values are delivered as a
            :class:`~torchkafka_amd.MXBatch` in the OCP Microscaling format -- blocks of 32 consecutive elements of
            the last dimension share one E8M0 scale byte; elements are ``float8_e4m3fn``, or e2m1 codes two per
            ``uint8`` -- made from the batch ``quantize=None`` would have delivered (same ``dtype``, ``normalize``,
            padding and ``pad_value``) by one more gfx950 launch (csrc/hip/mx_quant.hip), exactly
            ``quantize_mx(batch, quantize)``.  ``FixedWidth``: ``x`` becomes the ``MXBatch`` (with record fields
            ``(MXBatch, key, ...)``) and ``shape[-1]`` must be a multiple of 32; var-len / JSON:
            ``(MXBatch, lengths[, mask])`` and ``pad_to`` (or, with ``pad_to=None``, ``pad_multiple``) must be a
            multiple of 32.  The output dtype must be float32, bfloat16 or float16 (``TypeError`` otherwise, and
            for structured samples); ``layout`` must be ``"padded"``.
        drop_last: drop a final batch shorter than ``batch_size`` (DataLoader's meaning).
        return_info: yield ``(batch, BatchInfo)`` with each batch's partitions and offset ranges.
        native: use the native step driver (``False``: the Python loop, for debugging).
        multiprocessing_context: start method of the worker processes (``"fork"``, ``"spawn"``,
            ``"forkserver"``).
        commit_sink: ``"broker"`` (this process stores finished offsets into the synthetic broker),
            ``"worker"`` (each worker's consumer commits its own partitions, as the reference) or
            ``"auto"`` (broker when the workers read the synthetic broker with static sharding).
        rank: this process's rank for static sharding (default: torch.distributed's, else 0).
        world_size: ranks sharing the topic (default: torch.distributed's, else 1).
        timeout: seconds to wait for a batch before ``TimeoutError`` (0 waits forever).
        group_id: consumer group the commits go to (default: the one given to ``init_worker``).
        bootstrap_servers: where the group lives (default: the one given to ``init_worker``).
        base_seed: seed of the workers' RNGs (worker k gets ``base_seed + k``); None draws one from torch.
        decode: ``"device"`` (fixed-width / var-len records decoded by the gfx950 kernels straight from
            the pinned broker logs, CRC32C included; the workers only walk record headers),
            ``"host"`` (the workers CRC-check and pack the values) or ``"auto"`` (device when possible).
        json_parse: ``JsonArray`` records parsed by the gfx950 kernel (``"device"``), by the workers
            (``"host"``), or ``"auto"`` (device unless ``skip_bad=True`` needs rows dropped).
        bridge: ``"auto"``: workers pointed at a real Kafka cluster read a local replica that a native
            ``KafkaBridge`` fills with this rank's partitions (commits reach the cluster's coordinator);
            ``True`` requires it, ``False`` lets the workers' consumers read the cluster themselves.
        commit_on: ``"host"`` (commit when the next batch is requested, as the reference) or
            ``"device"`` (additionally wait until the GPU finished the user's work on the batch).
        commit: ``"async"`` (default: batch k's offsets are stored -- in the synthetic broker, or in a
            KafkaBridge replica that forwards them to the group coordinator within a few ms -- when
            batch k+1 is requested) or ``"sync"`` (the reference's semantics, kafka_dataset.py:130:
            batch k+1 is handed out only after batch k's device verdict landed, its offsets were
            stored and, through a bridge, the coordinator answered its OffsetCommit).  Under a
            cross-rank lockstep the same holds on every rank: before batch k+1 is taken, one
            agreement issued at step k+1 proves every rank finished batch k, and each rank commits
            its own part of batch k before it hands out k+1 (one collective per step).
        verify: ``"deliver"`` (a batch decoded or parsed on the GPU is handed out only once its
            kernel's verdict -- every RecordBatch's CRC32C, every JSON row's grammar -- landed; a
            corrupt batch raises ``CorruptRecordException`` before it is yielded, as kafka-python's
            ``check_crcs`` iterator raises before ``_process`` sees a record) or ``"commit"`` (the
            verdict gates only the commit: the batch may be yielded while its kernel still runs and
            the exception comes one or more steps later).  Host-decoded batches are verified by the
            workers before they are published, in both modes.
        lockstep: synchronise steps and commits across ranks when torch.distributed is initialised
            (``True``: when every rank of the group runs on this host, the node-local shared-memory
            transport (``csrc/core/shm_lockstep.h``: each rank writes its words into its own cache
            line, well under a microsecond per agreement); across hosts native RCCL on GPUs with an
            nccl group, the group's own all-reduce otherwise; ``"shm"`` / ``"rccl"`` / ``"host"`` (the
            group's all-reduce, e.g. gloo) force a transport, at any world size; ``"always"``: the
            automatic choice, also at world size 1).
        lockstep_depth: steps the per-step agreement is issued ahead (hides the collective's latency).
        lockstep_commit_every: async lockstep: finished batches become committable at least every
            this many steps (``Tuning.lockstep_commit_every``; None = per transport).
        h2d: ``"dma"`` (hipMemcpyAsync into device staging on ``copy_streams`` side streams, issued
            ``prefetch`` batches ahead), ``"zerocopy"`` (the collate kernel reads pinned host memory over
            PCIe: two HIP calls per batch instead of five, but the read runs on the compute stream) or
            ``"auto"`` (default: zero-copy for slots up to ``ZERO_COPY_MAX_BYTES``, where a batch is
            latency-bound; DMA above, where copy/compute overlap matters; var-len / JSON rows decoded
            on the device read an HBM mirror of the logs that the copy engines fill, fixed-width rows
            read the pinned logs in place -- loader/path_plan.py) or ``"direct"`` (experimental;
            fixed-width schemas on the synthetic broker: workers only locate each row in the broker log,
            the main process pins the logs in place and the collate kernel gathers rows straight out of
            them over PCIe, so no worker copies the payload.  Measured slower than "zerocopy" on MI355X
            (docs/PERFORMANCE.md): the CPU CRC pass still dominates a worker, the gather kernel pays a
            second dependent PCIe round trip, and pinning new log pages runs at ~13 GB/s).
        event_every: record a slot-completion event for one batch in k (default: ring slots / 4,
            at most 4); slots in between are released with the next event on the same stream.
        coalesce: fixed-width batches that are already staged when the next one is requested are
            collated together, up to this many per kernel launch (one allocation, one launch, one
            completion event); the following requests return them without a HIP call.  1 disables.
        coalesce_wait_us: while the GPU is still busy with an earlier launch, wait up to this long
            for enough staged batches to fill a group (costs no GPU time; a zero-copy batch takes
            7.1 us alone and 5.2 us in a group of 4).  0 launches whatever is staged at once.
        lockstep_timeout: seconds the native RCCL lockstep waits for the other ranks before it
            aborts its communicator and raises (a peer died or hung); <= 0 waits forever.
        numa_bind: before forking the workers, restrict this process (and so the workers) to the CPUs
            of the socket the target GPU is attached to (no-op on single-socket hosts or when
            ``TORCHKAFKA_NUMA=0``); see ``utils/topology.py``.
    """

    def __init__(self, dataset, batch_size: int = 256, *, num_workers: int = 4, worker_init_fn=None,
                 device=None, dtype: torch.dtype | None = None, config: LoaderConfig | dict | None = None,
                 **options):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if num_workers < 0:
            raise ValueError("num_workers must be >= 0")
        cfg = self.config = LoaderConfig.build(config, **options)
        tun = cfg.tuning
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.num_workers = int(num_workers)
        self.worker_init_fn = worker_init_fn
        if self.num_workers == 0:
            # the reference's single-process mode (auto_commit.py:49-58): the dataset was built with
            # its consumer in this process; a thread of this process packs the ring slots
            if getattr(dataset, "_consumer", None) is None:
                raise ValueError("DeviceLoader(num_workers=0) needs a dataset with its consumer, e.g. "
                                 "YourDataset('topic', bootstrap_servers=..., group_id=...), not a placeholder")
            if worker_init_fn is not None:
                raise ValueError("worker_init_fn is not used with num_workers=0 (there are no workers)")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.schema = getattr(dataset, "schema", None)
        self.dtype = dtype
        # behaviour (config.LoaderConfig)
        self.normalize = cfg.normalize
        self.sharding = cfg.sharding
        self.in_order = cfg.in_order
        self.drop_last = cfg.drop_last
        self.pad_to = cfg.pad_to
        self.pad_multiple = int(cfg.pad_multiple)
        self.pad_value = cfg.pad_value
        self.return_mask = cfg.return_mask
        self.layout = cfg.layout
        self.pack_to = None if cfg.pack_to is None else int(cfg.pack_to)
        self.return_ids = bool(cfg.return_ids)
        if self.layout == "packed" and getattr(self.schema, "kind", None) not in (1, 2):
            raise TypeError("layout='packed' needs a VarLen or JsonArray schema (fixed-width and structured "
                            "samples have no row lengths to pack)")
        self.seq_len = None if cfg.seq_len is None else int(cfg.seq_len)
        self.bins = None if cfg.bins is None else int(cfg.bins)
        if self.layout == "binned" and getattr(self.schema, "kind", None) not in (1, 2):
            raise TypeError("layout='binned' needs a VarLen or JsonArray schema (fixed-width and structured "
                            "samples have no row lengths to pack)")
        self._pad_bits: dict = {}
        # a Struct schema rides as its int32 carrier and is split behind the decode (_split); a dataset
        # with a _process of its own takes the per-record path, where the schema is not used
        self._struct = self.schema if isinstance(self.schema, Struct) and not self._process_overridden() else None
        if isinstance(self.schema, Struct):
            self._check_struct()
        self.quantize = cfg.quantize
        if self.quantize is not None:
            self._check_quantize()
        self.return_info = cfg.return_info
        self.native = cfg.native
        self.multiprocessing_context = cfg.multiprocessing_context
        self.commit_on = cfg.commit_on
        self.commit_mode = cfg.commit
        self.verify = cfg.verify
        self.commit_sink = cfg.commit_sink
        self.lockstep = cfg.lockstep
        self.lockstep_timeout = float(cfg.lockstep_timeout)
        self.lockstep_info: dict = {}  # how the last iteration agreed across ranks (bench / logs)
        self.h2d = cfg.h2d
        self.json_parse = cfg.json_parse
        self.decode = cfg.decode
        self.timeout = cfg.timeout
        r, w = dist_rank_world()
        self.rank = r if cfg.rank is None else int(cfg.rank)
        self.world_size = w if cfg.world_size is None else int(cfg.world_size)
        self.base_seed = (int(torch.empty((), dtype=torch.int64).random_().item()) if cfg.base_seed is None
                          else cfg.base_seed)
        # performance (config.Tuning)
        self.tuning = tun
        self.slots_per_worker = None if tun.slots_per_worker is None else int(tun.slots_per_worker)
        self.slot_bytes = tun.slot_bytes
        self.prefetch = int(tun.prefetch)
        self.copy_streams = int(tun.copy_streams)
        self.event_every = None if tun.event_every is None else int(tun.event_every)
        self.coalesce_wait_us = int(tun.coalesce_wait_us)
        self.lockstep_depth = None if tun.lockstep_depth is None else int(tun.lockstep_depth)
        self.lockstep_commit_every = (None if tun.lockstep_commit_every is None
                                      else int(tun.lockstep_commit_every))
        self.numa_bind = bool(tun.numa_bind)
        self._bridges: list = []
        if self.num_workers > 0 and cfg.bridge is not False:
            self.worker_init_fn = self._bridge_cluster(self.worker_init_fn, forced=cfg.bridge is True)
        self._group_id, self._servers = self._resolve_commit_target(cfg.group_id, cfg.bootstrap_servers)
        self._sink = self._resolve_sink()
        self.plan = PathPlan.build(
            device_type=self.device.type, schema=self.schema, native=self.native, decode=self.decode, h2d=self.h2d,
            json_parse=self.json_parse, synthetic_commits=self._commit_target_url()[0] != "",
            process_overridden=self._process_overridden(), return_info=self.return_info,
            drop_last=self.drop_last, json_count_mode=getattr(tun, "json_count", "auto"))
        # fixed-width device decode: 6 batches per launch; JSON / var-len and the host paths: 8
        # 6 for plain fixed-width device decode; 8 when the rows carry record fields (Key / Timestamp
        # columns: label 44-48 M against 38-40 M with 6, profiles/r06_s4) and for everything else
        self.coalesce = (int(tun.coalesce) if tun.coalesce is not None
                         else 6 if self.plan.span and not self._n_extras() else 8)
        self._pending_wms: list = []   # finished-but-uncommitted watermark lists
        self._committed: dict[int, int] = {}
        # state_dict(global_step=True): every partition's position after the batches handed out
        # (this loader's lifetime, and the checkpoint it resumed from) and how many steps that is
        self._delivered_pos: dict[int, int] = {}
        self._steps_delivered = 0
        self._global_step_base = 0
        self._norm = None
        self.stats = LoaderStats()
        self._run: _Run | None = None

    @property
    def n_producers(self) -> int:
        """Ring producers: the worker processes, or the in-process packer thread (num_workers=0)."""
        return max(1, self.num_workers)

    # ------------------------------------------------------------------ configuration helpers

    def _resolve_sink(self) -> str:
        """Where finished offsets are committed.  'broker': this process stores them straight into
        the synthetic broker's offset table (one native store per batch) -- only valid when the
        workers are simple (manually assigned) consumers of a synthetic broker.  'worker': each
        worker's own consumer commits them: required with sharding='group' (a member's commit is
        tied to its generation) and with any other consumer (kafka-python)."""
        synthetic = self._commit_target_url()[0] != ""
        if self.commit_sink == "broker":
            if not synthetic or self.sharding != "static":
                raise ValueError("commit_sink='broker' needs the synthetic broker, a group_id and sharding='static'")
            return "broker"
        if self.commit_sink == "worker" or self.sharding == "group" or not synthetic:
            return "worker"
        return "broker"

    def _process_overridden(self) -> bool:
        """The dataset maps records with a ``_process`` of its own (reference kafka_dataset.py:159):
        the native schema packers and the device decode would bypass it, so the workers run the
        per-record loop and the batches take the generic path."""
        from ..models.kafka_dataset import KafkaDataset

        return type(self.dataset)._process is not KafkaDataset._process

    def _event_every(self, n_slots: int) -> int:
        """Slots per completion event: one ``hipEventRecord`` per batch costs ~1.3 µs of host time,
        so with a deep ring only every k-th batch records one (k <= n_slots / 4 keeps workers fed;
        measured on MI355X, config 2: k=1 21.5M, k=2 24.8M, k=4 29.1M records/s)."""
        if self.event_every is not None:
            return self.event_every
        return max(1, min(4, n_slots // 4))

    def _check_struct(self) -> None:
        """A Struct schema converts per field: the loader-wide conversions do not apply to it."""
        if self.dtype is not None or self.normalize is not None:
            raise TypeError("a Struct schema takes no loader dtype= / normalize=: set out= / normalize= on its fields")
        if self.config.quantize is not None:
            raise TypeError(f"quantize={self.config.quantize!r}: a Struct batch is a dict of field tensors, not one "
                            "values tensor to quantise")
        if self.layout != "padded":
            raise TypeError(f"layout={self.layout!r} needs a VarLen or JsonArray schema (a Struct batch is a dict of "
                            "fixed-shape field tensors)")

    def _check_quantize(self) -> None:
        """``quantize=`` needs a float batch whose last dimension is cut into whole blocks of 32."""
        s, q = self.schema, self.quantize
        kind = getattr(s, "kind", None)
        if kind not in (0, 1, 2):
            raise TypeError(f"quantize={q!r} needs a FixedWidth, VarLen or JsonArray schema (structured samples "
                            "have no single values tensor to quantise)")
        out = self._out_dtype(torch.float32 if kind == 2 else s.dtype)
        if out not in (torch.float32, torch.bfloat16, torch.float16):
            raise TypeError(f"quantize={q!r} needs a float32, bfloat16 or float16 batch, not {out} "
                            "(set dtype=, or use a float schema)")
        if kind == 0:
            if not s.shape or s.shape[-1] % MX_BLOCK:
                raise ValueError(f"quantize={q!r}: the schema's last dimension must be a multiple of {MX_BLOCK}, "
                                 f"got shape {tuple(s.shape)}")
        elif (self.pad_to if self.pad_to is not None else self.pad_multiple) % MX_BLOCK:
            raise ValueError(f"quantize={q!r}: pad_to (or, with pad_to=None, pad_multiple) must be a multiple of "
                             f"{MX_BLOCK}")

    def _default_src_code(self) -> int:
        s = self.schema
        if s is None:
            return -1
        if getattr(s, "kind", None) == 2:
            return DTYPE_CODE[torch.float32]
        return DTYPE_CODE[s.dtype]

    def _slots_per_worker(self) -> int:
        if self.slots_per_worker is not None:
            return self.slots_per_worker
        try:
            rccl = self._lockstep_transport() == "rccl"
        except Exception:  # noqa: BLE001 - no process group to ask: no lockstep
            rccl = False
        return self.plan.slots_per_worker(self._slot_capacity(), self.n_producers, deep=rccl)

    def _n_extras(self) -> int:
        """Record-field columns (Key / Timestamp) the schema adds beside the value."""
        return len(getattr(self.schema, "fields", ()) or ())

    def _slot_capacity(self) -> int:
        if self.slot_bytes is not None:
            return int(self.slot_bytes)
        # record fields ride after the layout: one int64 per row each (+ alignment)
        nx = self._n_extras()
        return self.plan.layout_capacity(self.batch_size, self.schema) + (self.batch_size * 8 * nx + 256 if nx else 0)

    def _worker_cfg(self) -> dict:
        return {"batch_size": self.batch_size, "sharding": self.sharding, "rank": self.rank,
                "world_size": self.world_size, "native": self.native, "base_seed": self.base_seed,
                "gather": self.plan.direct, "json_device": self.plan.json_device, "json_count": self.plan.json_count,
                "span": self.plan.device_decode,
                "process_overridden": self.plan.process_overridden, "commit_table": None,
                "worker_spin_us": int(self.tuning.worker_spin_us), "in_process": False,
                "commit_mode": self.commit_mode}

    def _rank_partitions(self) -> list[int]:
        """Broker partition indices this rank's workers will read (static sharding of the topics
        given to ``init_worker``); empty when not known up front (group sharding, custom init)."""
        from ..models.kafka_dataset import _WorkerInit
        from ..parallel.sharding import shard_partitions

        wi = self.worker_init_fn
        if self.num_workers == 0:
            cons = getattr(self.dataset, "_consumer", None)
            topics = sorted(cons.subscription() or []) if cons is not None and hasattr(cons, "subscription") else []
        else:
            topics = list(wi.args) if isinstance(wi, _WorkerInit) else []
        if self.sharding != "static" or not topics:
            return []
        try:
            b = self._broker()
            out = []
            for topic in topics:
                if isinstance(topic, str) and b.has_topic(topic):
                    _, n, first = b.topic(topic)
                    out += [first + p for p in shard_partitions(n, self.rank, self.world_size)]
            return out
        except Exception:  # noqa: BLE001 - not a synthetic broker: pinned lazily, batch by batch
            return []

    def _out_dtype(self, src: torch.dtype) -> torch.dtype:
        if self.dtype is not None:
            return self.dtype
        return src

    def __len__(self):
        raise TypeError("a Kafka stream has no length")

    # ------------------------------------------------------------------ iteration
    def __iter__(self):
        return self._iterate(auto_commit=False)

    def _iterate(self, auto_commit: bool, process_group=None):
        if self._run is not None and not self._run.closed:
            raise RuntimeError("DeviceLoader is already being iterated")
        # fork the workers first: the lockstep below initialises HIP in this process
        run = self._run = _Run(self)
        lock = None
        try:
            transport = self._lockstep_transport(process_group, probe=True)
            if transport is not None:
                import torch.distributed as dist

                if dist.is_available() and dist.is_initialized():
                    if run.driver is not None:
                        if transport == "rccl":
                            run.rccl = self._make_rccl_lockstep(process_group)
                        elif transport == "shm":
                            run.rccl = self._make_shm_lockstep(process_group, hip())
                        else:
                            run.rccl = hip().PyLockstep(_host_allreduce_min(process_group))
                            self.lockstep_info = {"transport": "host", "backend": dist.get_backend(process_group),
                                                  "world_size": dist.get_world_size(process_group)}
                        every = self._lockstep_commit_every(transport)
                        run.driver.enable_lockstep(run.rccl, self._lockstep_depth(transport), every)
                        self.lockstep_info["commit_every"] = every
                        self.lockstep_info["depth"] = self._lockstep_depth(transport)
                    else:
                        from ..parallel.lockstep import Lockstep

                        shm = self._make_shm_lockstep(process_group, core()) if transport == "shm" else None
                        lock = Lockstep(process_group, None, transport=shm)
                        if shm is None:
                            self.lockstep_info = {"transport": "host", "backend": dist.get_backend(process_group),
                                                  "world_size": lock.world_size}
        except BaseException:
            run.close()
            raise
        if run.driver is not None:
            plan = self.stream_plan()
            if self.lockstep_info:
                self.lockstep_info["streams"] = plan
            if plan["shared"]:
                # measured: the lockstep on a shared normal-priority queue came back in ~60 µs, on a
                # queue of its own at the greatest priority in ~110 µs (profiles/r05_s19_rccl_matrix)
                log.debug("DeviceLoader: %d HIP streams on %d hardware queues (%s): some share a queue",
                          plan["total"], plan["hw_queues"], plan)
            yield from self._iterate_native(run, auto_commit)
            return
        finished = self._pending_wms
        prev = None
        step = 0
        completed = False
        try:
            sync = auto_commit and self.commit_mode == "sync"
            while True:
                item = self._next_item(run)
                status, fatal = 2, None
                if prev is not None and auto_commit:
                    finished.append(self._finish_marker(prev))  # the user is done with the previous batch
                    prev = None
                    if sync:
                        # commit='sync': batch k committed (and answered) BEFORE the agreement that
                        # hands out k+1, which carries how it went to every rank
                        try:
                            status = self._sync_commit_py()
                        except Exception as e:  # noqa: BLE001 - re-raised after the agreement
                            fatal, status = e, 0
                if lock is not None:
                    t_agree = time.perf_counter_ns()
                    try:
                        ok = lock.agree(item is not None, step, status)
                    except Exception as e:
                        if fatal is not None:
                            raise fatal from e
                        raise
                    t_agree = time.perf_counter_ns() - t_agree
                    st = self.stats
                    st.lockstep_agreements += 1
                    st.lockstep_wait_ns += t_agree
                    st.lockstep_step_wait_max_ns = max(st.lockstep_step_wait_max_ns, t_agree)
                    if auto_commit and not sync:
                        self._commit_finished()
                    if not ok:
                        break
                else:
                    if fatal is not None:
                        raise fatal
                    if auto_commit:
                        self._commit_finished()
                    if item is None:
                        break
                batch, wms = item
                if auto_commit:
                    prev = wms
                else:
                    finished.append((wms, None))  # manual mode: commit() covers every yielded batch
                pos = self._delivered_pos
                for pidx, _first, nxt, _n in wms:
                    if nxt > pos.get(pidx, -1):
                        pos[pidx] = nxt
                self._steps_delivered += 1
                step += 1
                yield batch
            completed = True
        finally:
            if completed and auto_commit:
                if prev is not None:
                    finished.append(self._finish_marker(prev))
                if run.carry:
                    finished.append((run.carry, None))
                    run.carry = []
                if lock is not None:
                    lock.barrier()
                self._commit_finished(wait=True)
                if self.commit_mode == "sync":
                    self._sync_commit_py()
            run.close()

    # ------------------------------------------------------------------ native iteration
    def _iterate_native(self, run: _Run, auto_commit: bool):
        """GPU iteration through the native step driver: one loop for every schema.  A *stage*
        makes one batch per call -- ``(status, commit status, item)`` -- and the loop around it
        owns what they share: result codes, commit logging, ``commit='sync'``, the wait timeout and
        the end of the iteration (final commit, stats, ring teardown).  Stages:

        * fixed-width (``FixedWidth`` schemas): ONE argument-free native call per batch (finish +
          commit the previous batch, take the next slot, allocate on the current stream, decode --
          coalesced with staged batches);
        * var-len / JSON (``VarLen`` / ``JsonArray``): the same with the pad/stack or JSON parse;
        * slot (everything else: ``return_info``, ``drop_last``, a ``_process`` of its own): the
          driver hands out slots and Python collates them.
        """
        drv = run.driver
        debug = _ds_logger.isEnabledFor(logging.DEBUG)
        log_commits = debug and auto_commit
        native_ac = auto_commit and not log_commits  # with DEBUG the commit comes back to Python to be logged
        if self.plan.fast_path:
            step, py_commits = self._fixed_stage(drv, native_ac), False
        elif self.plan.varlen_fast:
            step, py_commits = self._varlen_stage(drv, native_ac), False
        else:
            step, py_commits = self._slot_stage(run, auto_commit, debug), True
        if _roctx_enabled():
            step = _traced_step(step)
        sync = auto_commit and self.commit_mode == "sync"
        drv.set_sync_commit(sync)
        verify = self.verify == "deliver"
        completed = delivered = False
        wait_since = None
        try:
            while True:
                fatal = None
                if sync and delivered:
                    # commit='sync': asking for batch k+1 finishes batch k -- its verdict, its store
                    # and the coordinator's answer come FIRST, then the lockstep agreement that
                    # hands out k+1 carries how that went, so no rank sees k+1 before every rank
                    # committed k (the reference's auto_commit.py:55-58 / kafka_dataset.py:130 as a
                    # cross-rank barrier)
                    drv.finish_delivered(_stream_ptr(self.device))
                    try:
                        status = self._sync_commit(drv, debug)
                    except Exception as e:  # noqa: BLE001 - re-raised after the agreement
                        fatal, status = e, 0
                    drv.set_commit_status(status)
                    if fatal is not None and not drv.lockstep_enabled:
                        raise fatal
                try:
                    r, cs, item = step()
                except Exception as e:
                    if fatal is not None:
                        raise fatal from e
                    raise
                if cs:
                    self._log_commit(cs, debug)
                if r > 0 and verify and py_commits and drv.verify_delivered() < 0:
                    r = -5  # the fast stages wait for the verdict natively and return -5 themselves
                if r == -5:
                    # the batch's CRC32C / grammar verdict is bad: it never reaches the user (the
                    # reference's records pass kafka-python's check_crcs before _process sees them,
                    # kafka_dataset.py:156-162); the batches finished before it are committed first
                    if auto_commit and delivered:
                        self._commit_native(drv, debug)
                    raise CorruptRecordException(drv.parse_error())
                if r > 0:
                    if delivered and log_commits and not py_commits and not sync:
                        self._commit_logged(drv)
                    delivered = True
                    wait_since = None
                    self._steps_delivered += 1
                    yield item
                elif r == -2:
                    break
                elif r == -3:
                    raise WorkerError(drv.error())
                elif r == -4:  # an earlier device-checked batch was corrupt (manual-commit mode)
                    raise CorruptRecordException(drv.parse_error())
                else:  # -1: nothing within the poll slice
                    run._check_workers_native()
                    if self.timeout > 0:
                        now = time.monotonic()
                        wait_since = now if wait_since is None else wait_since
                        if now - wait_since > self.timeout:
                            raise TimeoutError(f"DeviceLoader timed out after {self.timeout}s waiting for a batch")
            completed = True
        finally:
            try:
                drv.finish_delivered(_stream_ptr(self.device))
                if completed:
                    drv.finish_lockstep()
                drv.drain_fenced(True)
                if completed and auto_commit:
                    self._commit_native(drv, debug)
                    if sync:
                        self._sync_commit(drv, debug)
                elif not auto_commit:
                    # manual mode: keep every yielded batch committable by DeviceLoader.commit()
                    pend = drv.take_pending()
                    if pend:
                        self._pending_wms.append(([(p, 0, o, 0) for p, o in pend], None))
            finally:
                self._absorb_driver_stats(drv)
                self._absorb_delivered(drv)
                run.close()

    def _fixed_stage(self, drv, native_ac: bool):
        s = self.schema
        prm = self._norm_params(s.row_elems)
        shift, scale = (prm[0].data_ptr(), prm[1].data_ptr()) if prm is not None else (0, 0)
        nx = self._n_extras()
        drv.configure_fast(self.device.index, [self.batch_size, *s.shape], DTYPE_CODE[self._out_dtype(s.dtype)],
                           s.row_elems, shift, scale, native_ac, 100, self.coalesce > 1, nx,
                           self.verify == "deliver")
        if nx < 2 or s.column_order() == list(range(nx)):
            return self._struct_stage(self._quantized_stage(drv.fast_next))
        order = s.column_order()  # fields added timestamp first: the native columns are key-first
        native = drv.fast_next

        def step():
            r, cs, item = native()
            if item is not None:
                item = (item[0], *(item[1 + i] for i in order))
            return r, cs, item
        return self._quantized_stage(step)

    def _quantized_stage(self, native):
        """``native`` with the values of every item quantised (``quantize=``), as ``_varlen_stage``
        wraps ``relayout``: the native step ordered the current stream behind the decode before it
        handed the batch out, so the quantise kernel goes on that stream right behind it."""
        if self.quantize is None:
            return native
        quantize = self._quantize

        def step():
            r, cs, item = native()
            if item is not None:
                item = (quantize(item[0]), *item[1:]) if isinstance(item, tuple) else quantize(item)
            return r, cs, item
        return step

    def _struct_stage(self, native):
        """``native`` with every item -- the int32 carrier batch of a ``Struct`` schema -- split into
        its dict of field tensors, as ``_quantized_stage`` wraps ``_quantize``: the split kernel goes
        on the current stream right behind the decode the native step ordered it after."""
        if self._struct is None:
            return native
        split = self._split

        def step():
            r, cs, item = native()
            if item is not None:
                item = split(item)
            return r, cs, item
        return step

    def _varlen_stage(self, drv, native_ac: bool):
        src = CODE_DTYPE[self._default_src_code()]
        dst_dt = self._out_dtype(src)
        if (dst_dt in FLOAT_DTYPES) != (src in FLOAT_DTYPES) and src in FLOAT_DTYPES:
            raise TypeError(f"cannot collate {src} records to {dst_dt}")
        drv.configure_varlen(self.device.index, DTYPE_CODE[dst_dt], -1 if self.pad_to is None else int(self.pad_to),
                             self.pad_multiple, float(self.pad_value), bool(self.return_mask), native_ac, 100,
                             self.verify == "deliver")
        if self.layout == "padded":
            return self._quantized_stage(drv.varlen_fast_next)
        native, relayout = drv.varlen_fast_next, (self._pack if self.layout == "packed" else self._bin)

        def step():
            # the native step ordered the current stream behind the decode (wait_group) before it
            # handed the padded batch out, so the pack / bin kernels go on that stream right behind it
            r, cs, item = native()
            if item is not None:
                item = relayout(item[0], item[1])
            return r, cs, item
        return step

    def _slot_stage(self, run: _Run, auto_commit: bool, debug: bool):
        drv = run.driver
        state = {"delivered": False}

        def step():
            drv.finish_delivered(_stream_ptr(self.device))  # asking for the next batch finishes the previous one
            if auto_commit and state["delivered"]:
                self._commit_native(drv, debug)
            item = self._next_item_driver(run)
            if item is None:
                return -2, 0, None
            drv.deliver_last()
            state["delivered"] = True
            return 1, 0, item[0]
        return step

    def _next_item(self, run: _Run):
        """Returns (batch, watermarks) or None at end of stream."""
        if run.driver is not None:
            return self._next_item_driver(run)
        t0 = time.perf_counter_ns()
        if run.engine is not None:
            run.release_completed()
        # top up the device-side prefetch (H2D of upcoming batches overlaps the user's step)
        while len(run.staged) < self.prefetch + 1:
            got = run.acquire(block=False)
            if got is None:
                break
            run.staged.append(got)
        if not run.staged:
            got = run.acquire(block=True)
            if got is None:
                return None
            run.staged.append(got)
        g, summ, wms = run.staged.popleft()
        t1 = time.perf_counter_ns()
        n_rows = summ[0]
        if n_rows == 0 or (self.drop_last and n_rows < self.batch_size):
            # nothing to deliver: carry the consumed offsets into the next delivered batch
            if n_rows and run.engine is None:
                run.ring.main_release(g)
            run.carry.extend(wms)
            return self._next_item(run)
        batch = self._collate(run, g, summ, wms)
        if run.carry:
            wms = run.carry + wms
            run.carry = []
        self.stats.record_batch(n_rows, summ[2], t1 - t0, time.perf_counter_ns() - t1)
        return batch, wms

    def _next_item_driver(self, run: _Run):
        drv = run.driver
        t0 = time.perf_counter_ns()
        while True:
            res = drv.next_slot(100)
            r = res[0]
            if r == -2:
                return None
            if r == -3:
                raise WorkerError(drv.error())
            if r == -4:
                raise CorruptRecordException(drv.parse_error())
            if r == -1:
                run._check_workers_native()
                if self.timeout > 0 and time.perf_counter_ns() - t0 > self.timeout * 1e9:
                    raise TimeoutError(f"DeviceLoader timed out after {self.timeout}s waiting for a batch")
                continue
            _, n_rows, kind, max_len, total, src_code, shape, payload_bytes = res
            wms = drv.last_watermarks()
            if self.drop_last and n_rows < self.batch_size:
                drv.discard_last()     # consumed but not handed out: finished right away
                drv.deliver_last()
                drv.finish_delivered()
                continue
            break
        t1 = time.perf_counter_ns()
        if kind == core().PACK_TREE:  # structured samples: one copy of the slot, leaves are views
            self._refuse_quantized_tree()
            out = self._collate_tree(run, drv.last_slot, payload_bytes,
                                     lambda block: drv.copy_payload_last(_stream_ptr(self.device), block.data_ptr()))
            self.stats.record_batch(n_rows, payload_bytes, t1 - t0, time.perf_counter_ns() - t1)
            if self.return_info:
                return KafkaBatch(out, None, None, wms, sum(w[3] for w in wms)), wms
            return out, wms
        src_dt = CODE_DTYPE[src_code]
        dst_dt = self._out_dtype(src_dt)
        if (dst_dt in FLOAT_DTYPES) != (src_dt in FLOAT_DTYPES) and src_dt in FLOAT_DTYPES:
            raise TypeError(f"cannot collate {src_dt} records to {dst_dt}")
        dev = self.device
        stream = _stream_ptr(dev)
        lengths = mask = None
        # device-decode and log-gather slots are fixed-width batches too (MainDriver.collate_fixed)
        fixed = kind in (core().PACK_FIXED, core().PACK_RECORD_SPAN, core().PACK_GATHER_FIXED)
        if fixed:
            if not shape:
                shape = tuple(self.schema.shape)
            row = int(max_len) if max_len else 1
            out = torch.empty((n_rows, *shape), dtype=dst_dt, device=dev)
            prm = self._norm_params(row)
            shift, scale = (prm[0].data_ptr(), prm[1].data_ptr()) if prm is not None else (0, 0)
            nx = drv.last_extras
            ext = torch.empty((nx, n_rows), dtype=torch.int64, device=dev) if nx else None
            drv.collate_fixed_last(stream, DTYPE_CODE[dst_dt], out.data_ptr(), row, shift, scale,
                                   ext.data_ptr() if ext is not None else 0)
            if self.quantize is not None:
                out = self._quantize(out)
            elif self._struct is not None:
                out = self._split(out)
            if ext is not None and not self.return_info:
                out = self._with_fields(out, ext)
        else:
            L = self.pad_to if self.pad_to is not None else int(max_len)
            if self.pad_to is None and self.pad_multiple > 1:
                L = (L + self.pad_multiple - 1) // self.pad_multiple * self.pad_multiple
            out = torch.empty((n_rows, L), dtype=dst_dt, device=dev)
            lengths = torch.empty(n_rows, dtype=torch.int64, device=dev)
            mask = torch.empty((n_rows, L), dtype=torch.bool, device=dev) if self.return_mask else None
            W = drv.collate_varlen_last(stream, DTYPE_CODE[dst_dt], out.data_ptr(), L, float(self.pad_value),
                                        lengths.data_ptr(), mask.data_ptr() if mask is not None else 0,
                                        0 if self.pad_to is not None else max(1, self.pad_multiple))
            if W != L:  # device-counted JSON: L was the workers' bound, W the width the kernel chose
                out = out.view(-1)[:n_rows * W].view(n_rows, W)
                if mask is not None:
                    mask = mask.view(-1)[:n_rows * W].view(n_rows, W)
        if not fixed and self.layout != "padded":
            out, lengths = self._relayout(out, lengths), None
        elif not fixed and self.quantize is not None:
            out = self._quantize(out)
        self.stats.record_batch(n_rows, payload_bytes, t1 - t0, time.perf_counter_ns() - t1)
        n_rec = sum(w[3] for w in wms)
        if self.return_info:
            return KafkaBatch(out, lengths, mask, wms, n_rec), wms
        if lengths is None and not fixed:
            return out, wms
        if fixed:
            return out, wms
        return ((out, lengths, mask) if self.return_mask else (out, lengths)), wms

    # ------------------------------------------------------------------ collate
    def _collate_tree(self, run: _Run, g: int, payload_bytes: int, copy):
        """A PACK_TREE slot (loader/tree.py) -> the sample structure, leaves on the device."""
        from . import tree

        desc, data = tree.descriptor(run.ring.payload_view(g))
        fdt = self.dtype if self.dtype is not None and self.dtype.is_floating_point else None
        if self.device.type == "cuda":
            block = torch.empty(payload_bytes, dtype=torch.uint8, device=self.device)
            copy(block)
        else:
            block = torch.frombuffer(run.ring.payload_view(g), dtype=torch.uint8, count=payload_bytes).clone()
        return tree.unpack(desc, data, block, fdt)

    def _collate(self, run: _Run, g: int, summ, wms):
        n_rows, _flags, payload_bytes, voff, max_len, total, _w, kind, src_code = summ
        if kind == core().PACK_TREE:
            self._refuse_quantized_tree()

            def copy(block):
                run.engine.copy_raw(g, _stream_ptr(self.device), 0, block.data_ptr(), payload_bytes)
            out = self._collate_tree(run, g, payload_bytes, copy)
            if run.engine is None:
                run.ring.main_release(g)
            if self.return_info:
                return KafkaBatch(out, None, None, wms, sum(w[3] for w in wms))
            return out
        fixed = kind == core().PACK_FIXED
        if src_code >= 0:
            src_dt = CODE_DTYPE[src_code]
            shape = tuple(run.ring.slot_sample(g)[1]) if fixed else None
        else:
            s = self.schema
            src_dt = s.dtype if kind != core().PACK_JSON_F32 else torch.float32
            shape = tuple(s.shape) if fixed else None
        dst_dt = self._out_dtype(src_dt)
        if (dst_dt in FLOAT_DTYPES) != (src_dt in FLOAT_DTYPES) and src_dt in FLOAT_DTYPES:
            raise TypeError(f"cannot collate {src_dt} records to {dst_dt}")
        dev = self.device
        lengths = mask = ext = None
        if fixed:
            x_off, nx = run.ring.slot_extras(g)
            if nx:  # record fields beside the values: [nx, rows] int64 at x_off (read before the slot is released)
                ext = torch.empty((nx, n_rows), dtype=torch.int64, device=dev)
                if run.engine is not None:
                    run.engine.copy_raw(g, _stream_ptr(dev), int(x_off), ext.data_ptr(), nx * n_rows * 8)
                else:
                    ext.copy_(torch.frombuffer(run.ring.payload_view(g), dtype=torch.int64, count=nx * n_rows,
                                               offset=int(x_off)).view(nx, n_rows))
            row = int(max_len) if max_len else 1
            out = torch.empty((n_rows, *shape), dtype=dst_dt, device=dev)
            prm = self._norm_params(row)
            if run.engine is not None:
                shift, scale = (prm[0].data_ptr(), prm[1].data_ptr()) if prm is not None else (0, 0)
                run.engine.collate_fixed(g, _stream_ptr(dev), voff, DTYPE_CODE[src_dt],
                                         out.data_ptr(), DTYPE_CODE[dst_dt], n_rows, row, shift, scale)
            else:
                view = run.ring.payload_view(g)
                src = torch.frombuffer(view, dtype=src_dt, count=n_rows * row, offset=voff).view(n_rows, *shape)
                if prm is None and dst_dt == src_dt:
                    # one memcpy: Tensor.copy_ would split 256 KiB over the intra-op threads, which
                    # contend with the spinning workers for the same cores (~0.3-0.8 ms per batch)
                    ctypes.memmove(out.data_ptr(), src.data_ptr(), out.numel() * out.element_size())
                elif prm is None:
                    out.copy_(src)
                else:
                    out.copy_(((src.reshape(n_rows, row).float() - prm[0]) * prm[1]).to(dst_dt).view(out.shape))
                run.ring.main_release(g)
        else:
            L = self.pad_to if self.pad_to is not None else int(max_len)
            if self.pad_to is None and self.pad_multiple > 1:
                L = (L + self.pad_multiple - 1) // self.pad_multiple * self.pad_multiple
            out = torch.empty((n_rows, L), dtype=dst_dt, device=dev)
            lengths = torch.empty(n_rows, dtype=torch.int64, device=dev)
            mask = torch.empty((n_rows, L), dtype=torch.bool, device=dev) if self.return_mask else None
            if run.engine is not None:
                run.engine.collate_varlen(g, _stream_ptr(dev), voff, DTYPE_CODE[src_dt],
                                          out.data_ptr(), DTYPE_CODE[dst_dt], n_rows, L, float(self.pad_value),
                                          lengths.data_ptr(), mask.data_ptr() if mask is not None else 0)
            else:
                from ..ops.collate import reference_varlen

                view = run.ring.payload_view(g)
                offs = torch.frombuffer(view, dtype=torch.int32, count=n_rows + 1).clone()
                vals = torch.frombuffer(view, dtype=src_dt, count=int(total), offset=voff).clone() if total else \
                    torch.empty(0, dtype=src_dt)
                res = reference_varlen(offs, vals, dst_dt, L, self.pad_value, self.return_mask)
                out.copy_(res[0])
                lengths.copy_(res[1])
                if mask is not None:
                    mask.copy_(res[2])
                run.ring.main_release(g)
        if not fixed and self.layout != "padded":
            out, lengths = self._relayout(out, lengths), None
        elif self.quantize is not None:
            out = self._quantize(out)
        elif fixed and self._struct is not None:
            out = self._split(out)
        n_rec = sum(w[3] for w in wms)
        if self.return_info:
            return KafkaBatch(out, lengths, mask, wms, n_rec)
        if fixed:
            return out if ext is None else self._with_fields(out, ext)
        if lengths is None:
            return out
        return (out, lengths, mask) if self.return_mask else (out, lengths)

    def _relayout(self, out: torch.Tensor, lengths: torch.Tensor) -> PackedBatch | BinnedBatch:
        """The post-layout step of every var-len route: a delivered padded batch -> the batch in
        ``self.layout`` ("packed" or "binned"), launched on the current stream (the stream the batch
        is delivered on; every route has ordered it behind the decode by now).

        The padded tensor and its lengths are dropped when this returns.  That is safe for the same
        reason a user may drop a delivered batch right after launching work on it: a block the
        native step allocated on a decode stream was recorded on the delivery stream
        (torch_step.cpp alloc_group / alloc_json_group: recordStream), so the caching allocator
        hands it out again only after an event behind this launch; every other route allocates on
        the delivery stream itself, where reuse is ordered behind the launch by the stream."""
        return self._pack(out, lengths) if self.layout == "packed" else self._bin(out, lengths)

    def _quantize(self, out: torch.Tensor) -> MXBatch:
        """The post-pass of ``quantize=``: a delivered values tensor -> its MXBatch, by one launch on
        the current stream (csrc/hip/mx_quant.hip; ``reference_mx`` on the CPU).  It sits where
        ``_relayout`` sits, behind every decode route alike, and the tensor it read is dropped when
        it returns: safe for the reason ``_relayout`` gives."""
        if out.device.type != "cuda":
            return reference_mx(out, self.quantize)
        if out.numel() >= 1 << 31:
            raise ValueError(f"quantize={self.quantize!r}: a batch must have fewer than 2^31 elements")
        return mx_launch(out, MX_FORMATS[self.quantize], self.quantize)

    def _split(self, out: torch.Tensor) -> dict:
        """The post-pass of a ``Struct`` schema: the delivered int32 carrier batch ``[rows, size / 4]``
        -> the dict of field tensors, by one launch on the current stream whatever the number of
        fields (csrc/hip/struct_split.hip; ``reference_struct`` on the CPU).  It sits where
        ``_relayout`` and ``_quantize`` sit, behind every decode route alike, and the carrier batch is
        dropped when it returns: safe for the reason ``_relayout`` gives."""
        if out.device.type != "cuda":
            return reference_struct(out, self._struct)
        if out.shape[0] == 0 or out.numel() * 4 >= 1 << 31:
            return split_struct(out, self._struct)  # no launch / the ValueError that names the limit
        return struct_launch(out, self._struct)

    def _refuse_quantized_tree(self) -> None:
        if self.quantize is not None:
            raise TypeError(f"quantize={self.quantize!r}: structured samples have no single values tensor to quantise")

    def _bin(self, out: torch.Tensor, lengths: torch.Tensor) -> BinnedBatch:
        """A delivered padded batch -> its BinnedBatch (two launches, csrc/hip/bin.hip)."""
        rows, W = out.shape
        bins = rows if self.bins is None else self.bins
        if out.device.type != "cuda":
            return reference_binned(out, lengths, self.seq_len, bins, self.pad_value)
        if rows * W >= 1 << 31 or bins * self.seq_len >= 1 << 31:
            raise ValueError("layout='binned': rows * width and bins * seq_len must be below 2^31")
        bits = self._pad_bits.get(out.dtype)
        if bits is None:
            bits = self._pad_bits[out.dtype] = pad_bits(out.dtype, self.pad_value)
        return bin_launch(out, lengths, self.seq_len, bins, bits)  # above hip().BIN_MAX_ROWS rows: ValueError

    def _pack(self, out: torch.Tensor, lengths: torch.Tensor) -> PackedBatch:
        """A delivered padded batch -> its PackedBatch, by one launch (csrc/hip/pack.hip)."""
        rows, W = out.shape
        cap = rows * W if self.pack_to is None else self.pack_to
        if out.device.type != "cuda":
            return reference_packed(out, lengths, cap, self.pad_value, self.return_ids)
        if rows * W >= 1 << 31:
            raise ValueError("layout='packed': rows * width must be below 2^31")
        bits = self._pad_bits.get(out.dtype)
        if bits is None:
            bits = self._pad_bits[out.dtype] = pad_bits(out.dtype, self.pad_value)
        return pack_launch(out, lengths, cap, bits, self.return_ids)

    def _with_fields(self, out, ext):
        """(values, fields...) in the order the schema added them (native columns: key first)."""
        order = self.schema.column_order()
        return (out, *(ext[i] for i in order))

    def _norm_params(self, row: int):
        if self.normalize is None:
            return None
        if self._norm is None or self._norm[0].numel() != row:
            self._norm = normalize_params(self.normalize, row, self.device)
        return self._norm

    # ------------------------------------------------------------------ observability
    def ring_occupancy(self) -> dict:
        """Slots of the live iteration's ring by state: ``ready`` (published by a worker, not yet
        taken), ``inflight`` (taken by the main process: staged, collated ahead or still read by
        the GPU), ``filling`` and ``free``; ``prefilled`` = ready + inflight, the batches a timed
        region starting now would not have to wait for."""
        run = self._run
        if run is None or run.closed:
            return {"free": 0, "filling": 0, "ready": 0, "inflight": 0, "prefilled": 0, "n_slots": 0}
        free, filling, ready, inflight = run.ring.slot_states()
        return {"free": free, "filling": filling, "ready": ready, "inflight": inflight,
                "prefilled": ready + inflight, "n_slots": run.ring.n_slots}

    def reset_stats(self) -> None:
        """Zeroes the loader's counters (and the native driver's) -- e.g. after warm-up."""
        self.stats.reset()
        run = self._run
        if run is not None and run.driver is not None and not run.closed:
            run.driver.reset_stats()

    def stats_summary(self) -> dict:
        """Counters so far, including the native driver's (commits, worker fill times, blocking)."""
        run = self._run
        if run is not None and run.driver is not None and not run.closed:
            self._absorb_driver_stats(run.driver)
        return self.stats.summary()

    def close(self) -> None:
        if self._run is not None:
            self._run.close()
            self._run = None
        for br in reversed(getattr(self, "_bridges", [])):  # forwards the last commits, then drops replicas
            br.close()
        self._bridges = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
