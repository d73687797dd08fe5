// Padded [rows, W] + lengths -> the packed (cu_seqlens) layout, on gfx950.
//
//   values[cu[r] : cu[r+1]] = padded[r, : lengths[r]]      cu[r+1] = min(capacity, lengths[0] + .. + lengths[r])
//   values[cu[rows] : capacity] = pad                      *total  = the unclamped sum (int64)
//   position_ids / segment_ids (optional): i / r inside row r, 0 / -1 in the tail
//
// A byte mover: the padded batch is already in the output dtype, so the kernel is instantiated per
// element size (1, 2, 4, 8) and the pad value arrives as bits.
//
// One launch per batch (pack_rows_kernel<T, false>): a workgroup of four waves owns four rows, one
// wave each.  Nothing is passed between workgroups -- each one sums `lengths` itself (64-lane
// shuffles, then LDS across its waves) into the exclusive prefix of its first row and the grand
// total.  lengths[256] is 2 KiB and sits in L2; there are no atomics and nothing to spin on, so
// the result is deterministic.  That recompute is rows^2 / 4 loads over the grid, so above
// kPackFusedRows a single-workgroup scan (pack_scan_kernel) writes cu_seqlens and total first and
// pack_rows_kernel<T, true> reads them.
//
// A length below 0 counts as 0 and one above W as W: no row is read past its end.  Every store is
// below `capacity` elements of its output: a row is cut where the capacity ends, later rows are empty.
#include <hip/hip_runtime.h>

#include "collate.h"

#include <algorithm>
#include <string>

namespace tkh {

namespace {

constexpr int kPackThreads = 256;
constexpr int kPackWave = 64;
constexpr int kPackRows = kPackThreads / kPackWave;  // rows per workgroup, one wave each

__device__ __forceinline__ long long clamp_len(int64_t n, int64_t W) { return n < 0 ? 0 : (n > W ? W : n); }

__device__ __forceinline__ long long cap_at(long long x, long long capacity) { return x >= capacity ? capacity : x; }

// the sum over the wave's 64 lanes, in lane 0
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = kPackWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kPackWave);
  return v;
}

// cu[0] = 0, cu[i + 1] = min(capacity, clamped lengths[0..i]), *total = the unclamped sum.  One
// workgroup walks the rows 256 at a time: inclusive scan inside each wave, wave totals through LDS.
__global__ __launch_bounds__(kPackThreads) void pack_scan_kernel(const int64_t* __restrict__ lengths, int64_t rows,
                                                                  int64_t W, int64_t capacity,
                                                                  int32_t* __restrict__ cu,
                                                                  int64_t* __restrict__ total) {
  __shared__ long long wsum[kPackRows];
  const int t = int(threadIdx.x), lane = t & (kPackWave - 1), wave = t / kPackWave;
  long long carry = 0;
  for (int64_t base = 0; base < rows; base += kPackThreads) {
    const int64_t i = base + t;
    long long v = i < rows ? clamp_len(lengths[i], W) : 0;
#pragma unroll
    for (int o = 1; o < kPackWave; o <<= 1) {
      const long long u = __shfl_up(v, o, kPackWave);
      if (lane >= o) v += u;
    }
    if (lane == kPackWave - 1) wsum[wave] = v;
    __syncthreads();
    long long before = carry, chunk = 0;
#pragma unroll
    for (int k = 0; k < kPackRows; ++k) {
      if (k < wave) before += wsum[k];
      chunk += wsum[k];
    }
    if (i < rows) cu[i + 1] = int32_t(cap_at(before + v, capacity));
    carry += chunk;
    __syncthreads();  // wsum is rewritten by the next chunk
  }
  if (t == 0) {
    cu[0] = 0;
    *total = carry;
  }
}

// kScanned: cu_seqlens and total were written by pack_scan_kernel on the same stream.
template <typename T, bool kScanned>
__global__ __launch_bounds__(kPackThreads) void pack_rows_kernel(const T* __restrict__ padded, int64_t rows, int64_t W,
                                                                  const int64_t* __restrict__ lengths,
                                                                  T* __restrict__ values, int64_t capacity, T pad,
                                                                  int32_t* cu, int64_t* __restrict__ total,
                                                                  int32_t* __restrict__ pos,
                                                                  int32_t* __restrict__ seg) {
  const int t = int(threadIdx.x), lane = t & (kPackWave - 1), wave = t / kPackWave;
  const int64_t first = int64_t(blockIdx.x) * kPackRows;  // workgroups past the last row only fill the tail
  const int64_t r = first + wave;
  long long begin = 0, end = 0, tail;
  if constexpr (kScanned) {
    tail = cu[rows];
    if (r < rows) {
      begin = cu[r];
      end = cu[r + 1];
    }
  } else {
    __shared__ long long part[2][kPackRows];
    long long before = 0, all = 0;
    for (int64_t i = t; i < rows; i += kPackThreads) {
      const long long n = clamp_len(lengths[i], W);
      all += n;
      if (i < first) before += n;
    }
    before = wave_sum(before);
    all = wave_sum(all);
    if (lane == 0) {
      part[0][wave] = before;
      part[1][wave] = all;
    }
    __syncthreads();
    before = all = 0;
#pragma unroll
    for (int k = 0; k < kPackRows; ++k) {
      before += part[0][k];
      all += part[1][k];
    }
    if (r < rows) {
      for (int64_t i = first; i < r; ++i) before += clamp_len(lengths[i], W);  // my workgroup's rows before mine
      begin = cap_at(before, capacity);
      end = cap_at(before + clamp_len(lengths[r], W), capacity);
      if (lane == 0) cu[r + 1] = int32_t(end);
    }
    tail = cap_at(all, capacity);
    if (blockIdx.x == 0 && t == 0) {
      cu[0] = 0;
      *total = all;
    }
  }
  if (r < rows) {
    const T* __restrict__ src = padded + r * W;
    const long long n = end - begin;  // <= W: the row is never read past its end
    for (long long i = lane; i < n; i += kPackWave) {
      values[begin + i] = src[i];
      if (pos != nullptr) {
        pos[begin + i] = int32_t(i);
        seg[begin + i] = int32_t(r);
      }
    }
  }
  const long long stride = (long long)gridDim.x * kPackThreads;
  for (long long i = tail + (long long)blockIdx.x * kPackThreads + t; i < capacity; i += stride) {
    values[i] = pad;
    if (pos != nullptr) {
      pos[i] = 0;
      seg[i] = -1;
    }
  }
}

template <typename T>
void launch_pack_t(const void* padded, int64_t rows, int64_t W, const int64_t* lengths, void* values, int64_t capacity,
                   uint64_t pad_bits, int32_t* cu, int64_t* total, int32_t* pos, int32_t* seg, hipStream_t stream) {
  // a workgroup per four rows; enough of them that a tail far larger than the rows is not left to a few
  const int64_t by_rows = (rows + kPackRows - 1) / kPackRows;
  const int64_t by_tail = std::min<int64_t>(256, (capacity + kPackThreads * 8 - 1) / (kPackThreads * 8));
  const dim3 grid(unsigned(std::max<int64_t>(1, std::max(by_rows, by_tail))));
  const T* src = static_cast<const T*>(padded);
  T* dst = static_cast<T*>(values);
  if (rows > kPackFusedRows) {
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(kPackThreads), 0, stream, lengths, rows, W, capacity, cu, total);
    hipLaunchKernelGGL((pack_rows_kernel<T, true>), grid, dim3(kPackThreads), 0, stream, src, rows, W, lengths, dst,
                       capacity, T(pad_bits), cu, total, pos, seg);
  } else {
    hipLaunchKernelGGL((pack_rows_kernel<T, false>), grid, dim3(kPackThreads), 0, stream, src, rows, W, lengths, dst,
                       capacity, T(pad_bits), cu, total, pos, seg);
  }
}

}  // namespace

void launch_pack_rows(const void* padded, int elem_size, int64_t rows, int64_t W, const int64_t* lengths, void* values,
                      int64_t capacity, uint64_t pad_bits, int32_t* cu, int64_t* total, int32_t* pos, int32_t* seg,
                      hipStream_t stream) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (rows < 0 || W < 0 || capacity < 0) throw std::invalid_argument("pack rows: negative rows, width or capacity");
  if (rows >= kLimit || W >= kLimit || rows * W >= kLimit || capacity >= kLimit)
    throw std::invalid_argument("pack rows: rows * width and capacity must be below 2^31 (cu_seqlens is int32)");
  if (cu == nullptr || total == nullptr) throw std::invalid_argument("pack rows: cu_seqlens and total are required");
  if ((rows > 0 && lengths == nullptr) || (rows * W > 0 && padded == nullptr) || (capacity > 0 && values == nullptr))
    throw std::invalid_argument("pack rows: null input or output");
  if ((pos == nullptr) != (seg == nullptr))
    throw std::invalid_argument("pack rows: position_ids and segment_ids come together");
  switch (elem_size) {
    case 1: launch_pack_t<uint8_t>(padded, rows, W, lengths, values, capacity, pad_bits, cu, total, pos, seg, stream); break;
    case 2: launch_pack_t<uint16_t>(padded, rows, W, lengths, values, capacity, pad_bits, cu, total, pos, seg, stream); break;
    case 4: launch_pack_t<uint32_t>(padded, rows, W, lengths, values, capacity, pad_bits, cu, total, pos, seg, stream); break;
    case 8: launch_pack_t<uint64_t>(padded, rows, W, lengths, values, capacity, pad_bits, cu, total, pos, seg, stream); break;
    default: throw std::invalid_argument("pack rows: element size must be 1, 2, 4 or 8 bytes");
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("pack rows launch: ") + hipGetErrorString(e));
}

}  // namespace tkh
