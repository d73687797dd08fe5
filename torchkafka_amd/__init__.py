"""torchkafka_amd: Kafka -> PyTorch streaming for AMD Instinct MI355X (gfx950).

Public API of Bendabir/torch-kafka (``KafkaDataset``, ``auto_commit``; reference
src/__init__.py:17-18) plus the MI355X device path (``DeviceLoader``), the
synthetic broker and a kafka-python compatible client.  ``import torchkafka``
is an alias of this package.
"""
import numpy.random  # noqa: F401  -- import eagerly: a lazy import racing a DataLoader fork deadlocks/crashes workers

from .config import LoaderConfig, Tuning
from .loader import DeviceLoader, KafkaBatch, auto_commit
from .models import Field, FixedWidth, JsonArray, KafkaDataset, Key, Struct, Timestamp, VarLen, WithFields
from .ops.collate import (BinnedBatch, MXBatch, PackedBatch, bin_padded, pack_padded, quantize_mx, reference_binned,
                          reference_mx, reference_packed, reference_struct, split_struct)

__version__ = "1.2.0+mi355x.7"

__all__ = ["KafkaDataset", "auto_commit", "DeviceLoader", "KafkaBatch", "PackedBatch", "BinnedBatch", "LoaderConfig",
           "Tuning", "FixedWidth", "VarLen", "JsonArray", "Key", "Timestamp", "WithFields", "SyntheticBroker",
           "KafkaBridge", "KafkaWireServer", "KafkaConsumer", "KafkaProducer", "TopicPartition",
           "ConsumerRebalanceListener", "pack_padded", "reference_packed", "bin_padded", "reference_binned", "MXBatch",
           "quantize_mx", "reference_mx", "Struct", "Field", "split_struct", "reference_struct"]


def __getattr__(name):
    if name in ("SyntheticBroker", "KafkaBridge", "KafkaWireServer"):
        from . import broker

        return getattr(broker, name)
    if name == "TopicPartition":
        from .client.records import TopicPartition

        return TopicPartition
    if name in ("KafkaConsumer", "KafkaProducer", "ConsumerRebalanceListener"):
        from . import client

        return getattr(client, name)
    raise AttributeError(name)
