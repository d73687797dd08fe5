// Host-side launchers of the gfx950 collate kernels (collate.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace tkh {

// Dense [rows, row] -> [rows, row] cast with optional fused (x - shift) * scale.
void launch_fixed(const void* src, int src_dt, void* dst, int dst_dt, int64_t rows, int64_t row, const float* shift,
                  const float* scale, hipStream_t stream);

// CSR (int32 offsets[rows+1] in elements, values 16B-aligned) -> padded
// [rows, L] with `pad`; optional int64 lengths[rows] and uint8 mask[rows, L].
void launch_varlen(const int32_t* offs, const void* vals, int src_dt, void* out, int dst_dt, int64_t rows, int64_t L,
                   double pad, int64_t* lengths, uint8_t* mask, hipStream_t stream);

// Up to kMaxGroup dense casts (consecutive batches, same dtypes and row width) in one launch.
// 8: JSON groups of 16 were tried (config 4: 35-36.6 M rec/s against 38.6-39.1 M for 8, even with
// a 32-deep ring: the first batch of a group waits longer for its parse kernel; profiles/r04_s6).
constexpr int kMaxGroup = 8;
// host_src: the sources are pinned host memory read over PCIe (zero-copy), which sizes the grid.
void launch_fixed_group(const void* const* srcs, int src_dt, void* const* dsts, int dst_dt, const int64_t* rows, int n,
                        int64_t row, const float* shift, const float* scale, hipStream_t stream, bool host_src);

// Fixed-width rows gathered from pinned broker logs: ents[k][i] = (pidx << 44) | byte offset,
// bases[pidx] = device address of partition pidx's log.  Rows of `row_bytes` at any alignment.
void launch_gather_group(const uint64_t* const* ents, int src_dt, void* const* dsts, int dst_dt, const int64_t* rows,
                         int n, const uint64_t* bases, int64_t row_bytes, const float* shift, const float* scale,
                         hipStream_t stream);

// JSON text rows (tk::JsonRowDesc[n_rows] + values area, kPackJsonText) parsed on the
// device -> padded [n_rows, L] float dtype; a row with a grammar error stores its index
// into *err (host-mapped, may be null) and gets NaN for the bad numbers.
using tk::JsonRowDesc;
void launch_json_rows(const JsonRowDesc* rows, const void* vals, void* out, int dst_dt, int64_t n_rows, int64_t L,
                      double pad, int64_t* lengths, uint8_t* mask, int32_t* err, hipStream_t stream);

// Up to kMaxGroup JSON batches in one launch; row_base[k] = first global row of batch k,
// row_base[n] = total rows.  Entries k >= n are ignored.
struct JsonGroupArgs {
  int n;
  float pad;
  int64_t row_base[kMaxGroup + 1];
  const JsonRowDesc* rows[kMaxGroup];
  const uint8_t* vals[kMaxGroup];
  void* out[kMaxGroup];
  int64_t L[kMaxGroup];
  int64_t* lengths[kMaxGroup];
  uint8_t* mask[kMaxGroup];
  int32_t* err[kMaxGroup];
  // kPackJsonSpan: bytes of each batch's staging area (a descriptor reaching beyond it is a bad
  // row, never read), and the tag OR-ed into a parse error's row index (tk::kSpanParseErrBit); a
  // parse error then never overwrites an earlier verdict (the stage kernel's CRC failure).
  uint64_t vals_cap[kMaxGroup];
  int32_t err_tag;
  // Device-counted batches (kSlotDevCount): L[k] is only the capacity of out/mask; the width is
  // min(L[k], the stage kernel's count rounded up to `mult`) (mult 0: L[k], a fixed pad_to width),
  // and the batch's first block stores {width, rows left to the host (0/1), 1} into the
  // host-mapped info[k] (MainDriver::json_width).  ctr[k]: the tagged count words
  // (JsonStageBatch::ctr), valid where their high half equals ctr_tag[k]; nullptr: L[k].
  const unsigned long long* ctr[kMaxGroup];
  uint32_t ctr_tag[kMaxGroup];
  int32_t trunc[kMaxGroup];  // json_count_kernel: rows keep at most this many elements (-1: all)
  int32_t* info[kMaxGroup];
  int32_t mult;
  // 1 (mult 0 only): no json_count_kernel ran -- each parse block counts its own device-counted
  // row and raises info[k][1] when it leaves the row to the host; json_report_kernel, launched
  // behind the parse on the same stream, stores the width and the done flag
  int32_t fused_count;
};
void launch_json_group(JsonGroupArgs& a, int dst_dt, hipStream_t stream);
// Device counting of a staged group (json_span.hip): before launch_json_group on the same stream.
void launch_json_count(const JsonGroupArgs& a, hipStream_t stream);

// Padded [rows, W] (any dtype of `elem_size` 1/2/4/8 bytes) + int64 lengths[rows] -> the packed layout
// (pack.hip): values[capacity] with the rows back to back and `pad_bits` behind them, int32
// cu[rows + 1] clamped to capacity, the unclamped int64 *total, and -- both or neither -- int32
// pos[capacity] / seg[capacity].  One launch up to kPackFusedRows rows, a scan launch before it above.
constexpr int64_t kPackFusedRows = 1024;
void launch_pack_rows(const void* padded, int elem_size, int64_t rows, int64_t W, const int64_t* lengths, void* values,
                      int64_t capacity, uint64_t pad_bits, int32_t* cu, int64_t* total, int32_t* pos, int32_t* seg,
                      hipStream_t stream);

// Padded [rows, W] + int64 lengths[rows] -> the binned layout (bin.hip): rows placed first-fit, in
// arrival order, into `bins` sequences of `seq_len` elements.  values / seg / pos are [bins, seq_len]
// (`pad_bits` / -1 / 0 where no row landed), int32 bin_lens[bins], row_bin / row_start / row_lens
// [rows] (-1 / -1 for a row that found no bin), *n_bins, *unplaced and the int64 *cut (elements of
// rows longer than seq_len).  Two launches: a one-workgroup plan (free[] in LDS, hence kBinMaxRows)
// and the move.
constexpr int kBinMaxRows = 16384;
void launch_bin_rows(const void* padded, int elem_size, int64_t rows, int64_t W, const int64_t* lengths,
                     int64_t seq_len, int64_t bins, void* values, uint64_t pad_bits, int32_t* seg, int32_t* pos,
                     int32_t* bin_lens, int32_t* row_bin, int32_t* row_start, int32_t* row_lens, int32_t* n_bins,
                     int32_t* unplaced, int64_t* cut, hipStream_t stream);

// A contiguous f32 / bf16 / f16 array of n_blocks * 32 elements (16-byte aligned) -> OCP MX
// (mx_quant.hip, rules in mx_block.h): `fmt` 0 = mxfp8, values[32 * n_blocks] e4m3fn bytes; 1 = mxfp4,
// values[16 * n_blocks] with two e2m1 codes per byte (element 2i in the low nibble); scales[n_blocks]
// E8M0 bytes, plain row-major.  `values` 16-byte aligned.  One launch of at most kMxMaxGrid workgroups.
constexpr int kMxMaxGrid = 2048;
void launch_mx_quantize(const void* src, int src_dt, int64_t n_blocks, int fmt, void* values, uint8_t* scales,
                        hipStream_t stream);

// Packed little-endian struct records raw[rows, record_bytes] (4-byte aligned) -> one dense tensor
// per field (struct_split.hip).  Field f is `elems` elements of `src_dt` at byte `src_off` of every
// record -- any byte offset; fields may leave gaps and may overlap -- and is written to
// dst[rows, elems] (aligned to its element size) as `dst_dt`: kStructCopy copies the bytes in the
// field's own dtype, f32 / f16 / bf16 / fp8 / i32 / i64 convert by convert.h (a float field has float
// destinations only).  shift / scale: device f32[elems], both or neither; float destinations only.
// The table travels by value in the kernel arguments; one launch for all fields.
constexpr int kStructMaxFields = 32;
constexpr int kStructMaxRecord = 32768;
constexpr int kStructCopy = -1;
struct StructField {
  int32_t src_off, elems;
  int32_t src_dt, dst_dt;
  void* dst;
  const float* shift;
  const float* scale;
};
struct StructTable {
  int32_t n;
  StructField f[kStructMaxFields];
};
// rows of a workgroup's tile: at most 64 and at most 32 KiB, halved down to 16 while the batch has
// fewer than 64 tiles
int struct_tile_rows(int64_t rows, int32_t record_bytes);
void launch_struct_split(const void* raw, int64_t rows, int32_t record_bytes, const StructTable& table,
                         hipStream_t stream);

std::vector<std::pair<std::string, double>> api_bench(int device, int iters);

}  // namespace tkh
