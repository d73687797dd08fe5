"""Native ops: host core (_tkcore) and gfx950 collate kernels (_tkhip)."""
from .native import build_info, core, hip, loaded_extensions

__all__ = ["build_info", "core", "hip", "loaded_extensions", "collate_fixed", "collate_varlen", "pack_padded",
           "bin_padded", "quantize_mx", "split_struct"]


def __getattr__(name):
    if name in ("collate_fixed", "collate_varlen", "reference_fixed", "reference_varlen", "pack_padded",
                "reference_packed", "PackedBatch", "bin_padded", "reference_binned", "BinnedBatch", "quantize_mx",
                "reference_mx", "MXBatch", "split_struct", "reference_struct"):
        from . import collate

        return getattr(collate, name)
    raise AttributeError(name)
