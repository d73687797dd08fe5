"""Dataset classes: the reference's KafkaDataset plus declarative record schemas."""
from .kafka_dataset import KafkaDataset
from .schema import Field, FixedWidth, JsonArray, Key, Struct, Timestamp, VarLen, WithFields

__all__ = ["KafkaDataset", "FixedWidth", "VarLen", "JsonArray", "Key", "Timestamp", "WithFields", "Struct", "Field"]
