// A batch of packed little-endian struct records, raw[rows, record_bytes], -> one dense tensor per
// field, on gfx950.  One launch for all fields.
//
//   field f    elems elements of src_dt at byte src_off of every record (any byte offset; fields may
//              leave gaps and may overlap), written to dst[rows, elems] as dst_dt: copied unchanged
//              (kStructCopy), or converted by the rules of convert.h (Conv: bit-exact with Tensor.to,
//              with the optional (x - shift[e]) * scale[e] on float destinations).
//
// A 256-thread workgroup takes a tile of R consecutive rows (R * record_bytes <= 32 KiB) and stages
// its bytes into LDS once: 16-byte global loads over the part of the tile that is 16-byte aligned,
// single dwords for the head and the tail (a tile starts on a 4-byte boundary, not always a 16-byte
// one), so nothing outside raw[0, rows * record_bytes) is read.  The LDS row pitch is the record's
// dwords made odd: a scalar field is read at a stride of one row, and an odd pitch spreads 32 rows
// over the 32 banks of a dword read where an even one folds them onto a few.
//
// The tile's work is cut into chunks of 64 (row, element) pairs, field after field, and dealt to the
// four waves in turn, so one wide field and 32 scalar fields both keep every wave busy.  Within a
// chunk consecutive lanes take consecutive pairs: they read consecutive elements of a row and store
// consecutive elements of the output.  The dtype switch is per field, hence wave-uniform.  An
// element is assembled from the aligned LDS dwords that hold it and a funnel shift by its byte
// offset; the dword read past an element that ends on a boundary is shifted out (the LDS image has
// one spare dword behind the last row for it).
#include <hip/hip_runtime.h>

#include "collate.h"
#include "convert.h"

#include <algorithm>
#include <string>

namespace tkh {

namespace {

constexpr int kSplitThreads = 256;
constexpr int kSplitWaves = kSplitThreads / 64;
constexpr int kSplitTileBytes = 32 << 10;
constexpr int kSplitMaxRows = 64;

// dtypes.h's dtype_size, for both sides
__host__ __device__ constexpr int split_size(int dt) {
  return (dt == kF32 || dt == kI32) ? 4 : (dt == kF16 || dt == kBF16) ? 2 : dt == kI64 ? 8 : 1;
}

template <int kBytes> struct Bits;
template <> struct Bits<1> { using type = uint8_t; };
template <> struct Bits<2> { using type = uint16_t; };
template <> struct Bits<4> { using type = uint32_t; };
template <> struct Bits<8> { using type = uint64_t; };

// the kBytes bytes at byte address `a` of the LDS image
template <int kBytes>
__device__ __forceinline__ typename Bits<kBytes>::type lds_bits(const uint32_t* __restrict__ lds, uint32_t a) {
  if constexpr (kBytes == 1) {
    return reinterpret_cast<const uint8_t*>(lds)[a];
  } else {
    const uint32_t d = a >> 2, sh = (a & 3u) * 8u;
    const uint64_t lo = (uint64_t(lds[d + 1]) << 32) | lds[d];
    if constexpr (kBytes == 8) {
      const uint64_t hi = (uint64_t(lds[d + 2]) << 32) | lds[d + 1];
      return (uint64_t(uint32_t(hi >> sh)) << 32) | uint32_t(lo >> sh);
    } else {
      return typename Bits<kBytes>::type(lo >> sh);
    }
  }
}

// The chunks first, first + kSplitWaves, ... (below n_chunks) of one field of the tile: pair p is
// element p % elems of tile row p / elems, and lands at out[p] (`out` = the tile's first row).
template <typename S, typename D, bool kCopy>
__device__ __forceinline__ void split_field(const uint32_t* __restrict__ lds, const StructField& f, void* out,
                                            uint32_t pairs, uint32_t first, uint32_t n_chunks, uint32_t pitch_bytes,
                                            uint32_t lane) {
  using B = typename Bits<sizeof(S)>::type;
  const uint32_t elems = uint32_t(f.elems);
  const bool affine = f.shift != nullptr;
  for (uint32_t c = first; c < n_chunks; c += kSplitWaves) {
    const uint32_t p = c * 64u + lane;
    if (p >= pairs) break;  // the last chunk of a field may be partial
    const uint32_t r = elems == 1 ? p : p / elems, e = p - r * elems;
    const B bits = lds_bits<sizeof(S)>(lds, r * pitch_bytes + uint32_t(f.src_off) + e * uint32_t(sizeof(S)));
    if constexpr (kCopy) {
      static_cast<B*>(out)[p] = bits;
    } else {
      const S s = __builtin_bit_cast(S, bits);
      const float shift = affine ? f.shift[e] : 0.0f, scale = affine ? f.scale[e] : 1.0f;
      static_cast<D*>(out)[p] = Conv<S, D, IsIntDst<D>::value>::apply(s, shift, scale, affine);
    }
  }
}

#define TK_SPLIT_ARGS lds, f, out, pairs, first, n_chunks, pitch_bytes, lane
#define TK_SPLIT_FLOAT_DST(S)                                           \
  case kF32: split_field<S, float, false>(TK_SPLIT_ARGS); break;        \
  case kF16: split_field<S, _Float16, false>(TK_SPLIT_ARGS); break;     \
  case kBF16: split_field<S, __bf16, false>(TK_SPLIT_ARGS); break;      \
  case kFP8E4M3: split_field<S, fp8e4m3, false>(TK_SPLIT_ARGS); break;
#define TK_SPLIT_INT_DST(S)                                             \
  case kI32: split_field<S, int32_t, false>(TK_SPLIT_ARGS); break;      \
  case kI64: split_field<S, int64_t, false>(TK_SPLIT_ARGS); break;
// a float source has float destinations only (the launcher refuses the rest)
#define TK_SPLIT_FLOAT_SRC(S) \
  switch (f.dst_dt) { TK_SPLIT_FLOAT_DST(S) default: break; }
#define TK_SPLIT_INT_SRC(S) \
  switch (f.dst_dt) { TK_SPLIT_FLOAT_DST(S) TK_SPLIT_INT_DST(S) default: break; }

__global__ __launch_bounds__(kSplitThreads) void struct_split_kernel(const uint32_t* __restrict__ raw, int64_t rows,
                                                                      uint32_t rec_dw, uint32_t tile_rows,
                                                                      const StructTable table) {
  extern __shared__ uint32_t lds[];  // [tile_rows][pitch] + 1 spare dword
  const uint32_t tid = threadIdx.x;
  const int64_t row0 = int64_t(blockIdx.x) * tile_rows;
  const uint32_t rt = rows - row0 < int64_t(tile_rows) ? uint32_t(rows - row0) : tile_rows;  // rows of this tile: >= 1
  const uint32_t pitch = rec_dw | 1u;
  const uint32_t tile_dw = rt * rec_dw;  // <= 8192

  // ---- stage raw[row0 .. row0 + rt) into LDS: dword w of the tile -> lds[(w / rec_dw) * pitch + w % rec_dw]
  const uint32_t* __restrict__ g = raw + row0 * rec_dw;
  const uint32_t to16 = (4u - (uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u)) & 3u;  // dwords up to a 16-byte boundary
  const uint32_t head = to16 < tile_dw ? to16 : tile_dw;
  const uint32_t body = (tile_dw - head) / 4u;  // 16-byte loads
  const uint32_t tail0 = head + body * 4u;      // the first dword of the tail; tile_dw - tail0 < 4
  if (tid < head) {
    lds[(tid / rec_dw) * pitch + tid % rec_dw] = g[tid];
  } else if (tid < head + (tile_dw - tail0)) {
    const uint32_t w = tail0 + (tid - head);
    lds[(w / rec_dw) * pitch + w % rec_dw] = g[w];
  }
  const uint4* __restrict__ g16 = reinterpret_cast<const uint4*>(g + head);
  for (uint32_t q = tid; q < body; q += kSplitThreads) {
    const uint4 v = g16[q];
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
    const uint32_t w = head + q * 4u;
    uint32_t r = w / rec_dw, c = w - r * rec_dw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // the four dwords may cross a row end (more than once below 4-dword records)
      lds[r * pitch + c] = x[k];
      if (++c == rec_dw) c = 0, ++r;
    }
  }
  __syncthreads();

  // ---- the fields, cut into chunks of 64 pairs that the waves take in turn
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6)));
  const uint32_t lane = tid & 63u;
  const uint32_t pitch_bytes = pitch * 4u;
  uint32_t turn = 0;  // (chunks dealt so far) % kSplitWaves
  for (int fi = 0; fi < table.n; ++fi) {
    const StructField f = table.f[fi];
    const uint32_t pairs = rt * uint32_t(f.elems);  // <= 32 KiB of source per tile: <= 32768
    const uint32_t n_chunks = (pairs + 63u) / 64u;
    const uint32_t first = (wave + kSplitWaves - turn) % kSplitWaves;
    turn = (turn + n_chunks) % kSplitWaves;
    if (first >= n_chunks) continue;
    void* out = static_cast<char*>(f.dst) + row0 * f.elems * int64_t(split_size(f.dst_dt == kStructCopy ? f.src_dt : f.dst_dt));
    if (f.dst_dt == kStructCopy) {
      switch (split_size(f.src_dt)) {
        case 1: split_field<uint8_t, uint8_t, true>(TK_SPLIT_ARGS); break;
        case 2: split_field<uint16_t, uint16_t, true>(TK_SPLIT_ARGS); break;
        case 4: split_field<uint32_t, uint32_t, true>(TK_SPLIT_ARGS); break;
        case 8: split_field<uint64_t, uint64_t, true>(TK_SPLIT_ARGS); break;
        default: break;
      }
      continue;
    }
    switch (f.src_dt) {
      case kF32: TK_SPLIT_FLOAT_SRC(float) break;
      case kF16: TK_SPLIT_FLOAT_SRC(_Float16) break;
      case kBF16: TK_SPLIT_FLOAT_SRC(__bf16) break;
      case kU8: TK_SPLIT_INT_SRC(uint8_t) break;
      case kI8: TK_SPLIT_INT_SRC(int8_t) break;
      case kI32: TK_SPLIT_INT_SRC(int32_t) break;
      case kI64: TK_SPLIT_INT_SRC(int64_t) break;
      default: break;
    }
  }
}

bool split_source(int dt) {
  return dt == kF32 || dt == kF16 || dt == kBF16 || dt == kU8 || dt == kI8 || dt == kI32 || dt == kI64;
}

}  // namespace

int struct_tile_rows(int64_t rows, int32_t record_bytes) {
  int r = std::max(1, std::min(kSplitMaxRows, kSplitTileBytes / record_bytes));
  // few rows: smaller tiles, so that a batch of a few hundred records still spreads over the CUs
  while (r >= 32 && (rows + r - 1) / r < 64) r >>= 1;
  return r;
}

void launch_struct_split(const void* raw, int64_t rows, int32_t record_bytes, const StructTable& table,
                         hipStream_t stream) {
  const std::string w = "struct split: ";
  if (table.n < 1 || table.n > kStructMaxFields)
    throw std::invalid_argument(w + "1 to " + std::to_string(kStructMaxFields) + " fields");
  if (record_bytes < 4 || record_bytes % 4 != 0 || record_bytes > kStructMaxRecord)
    throw std::invalid_argument(w + "record_bytes must be a multiple of 4 in [4, " + std::to_string(kStructMaxRecord) +
                                "]");
  if (rows < 0 || rows * int64_t(record_bytes) >= (int64_t(1) << 31))
    throw std::invalid_argument(w + "rows * record_bytes must be in [0, 2^31)");
  for (int i = 0; i < table.n; ++i) {
    const StructField& f = table.f[i];
    const std::string fw = w + "field " + std::to_string(i) + ": ";
    if (!split_source(f.src_dt)) throw std::invalid_argument(fw + "unsupported source dtype");
    const int ssize = dtype_size(f.src_dt);
    if (f.dst_dt != kStructCopy) {
      if (f.dst_dt != kF32 && f.dst_dt != kF16 && f.dst_dt != kBF16 && f.dst_dt != kFP8E4M3 && f.dst_dt != kI32 &&
          f.dst_dt != kI64)
        throw std::invalid_argument(fw + "unsupported destination dtype");
      if (is_float_dt(f.src_dt) && !is_float_dt(f.dst_dt))
        throw std::invalid_argument(fw + "a float field has no integer destination");
    }
    if ((f.shift == nullptr) != (f.scale == nullptr))
      throw std::invalid_argument(fw + "shift and scale come together");
    if (f.shift != nullptr && (f.dst_dt == kStructCopy || !is_float_dt(f.dst_dt)))
      throw std::invalid_argument(fw + "normalisation needs a float destination");
    if (f.src_off < 0 || f.elems < 1 || int64_t(f.src_off) + int64_t(f.elems) * ssize > record_bytes)
      throw std::invalid_argument(fw + "the field does not lie inside the record");
    if (rows == 0) continue;
    if (f.dst == nullptr) throw std::invalid_argument(fw + "null output");
    const int dsize = f.dst_dt == kStructCopy ? ssize : dtype_size(f.dst_dt);
    if (reinterpret_cast<uintptr_t>(f.dst) % dsize != 0)
      throw std::invalid_argument(fw + "the output must be aligned to its element size");
  }
  if (rows == 0) return;
  if (raw == nullptr) throw std::invalid_argument(w + "null input");
  if (reinterpret_cast<uintptr_t>(raw) % 4 != 0) throw std::invalid_argument(w + "the input must be 4-byte aligned");
  const int tile_rows = struct_tile_rows(rows, record_bytes);
  const uint32_t rec_dw = uint32_t(record_bytes / 4);
  const size_t lds_bytes = (size_t(tile_rows) * (rec_dw | 1u) + 1) * 4;  // <= 32 KiB + 64 pad dwords + 1
  const int64_t tiles = (rows + tile_rows - 1) / tile_rows;              // < 2^29
  hipLaunchKernelGGL(struct_split_kernel, dim3(unsigned(tiles)), dim3(kSplitThreads), lds_bytes, stream,
                     static_cast<const uint32_t*>(raw), rows, rec_dw, uint32_t(tile_rows), table);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(w + "launch: " + hipGetErrorString(e));
}

}  // namespace tkh
