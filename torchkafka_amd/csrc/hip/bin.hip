// Padded [rows, W] + lengths -> the binned layout: several rows packed into each fixed-length
// sequence of a [bins, seq_len] batch by first-fit in arrival order, on gfx950.
//
//   free[b] = seq_len
//   for r in order:  n = min(clamp(lengths[r], 0, W), seq_len)     (cut += what min() took off)
//                    b = the lowest bin with free[b] >= n, none: row_bin = row_start = -1, unplaced += 1
//                    row_bin[r] = b, row_start[r] = seq_len - free[b], free[b] -= n
//   values[b, start : start + n] = padded[r, : n]; segment_ids = r, position_ids = 0 .. n-1 there
//   every other cell: values = pad, segment_ids = -1, position_ids = 0
//   bin_lens[b] = seq_len - free[b], n_bins = the number of bins with bin_lens > 0 (a prefix)
//
// A byte mover, as pack.hip: instantiated per element size (1, 2, 4, 8), the pad value arrives as bits.
//
// Two launches on one stream.  bin_plan_kernel is one workgroup: first-fit is sequential over the
// rows but parallel over the bins, so free[] sits in LDS and, for each row, the first wave tests 64
// consecutive bins per step (bin base + lane, base a multiple of 64) and ballots.  Bin b is read
// and written by lane b % 64 alone, so no LDS word ever passes between lanes inside the loop, and
// each lane keeps the word of the 64-bin block it tested last in a register, written back when
// the search moves to another block: while a batch needs no more than 64 bins a row costs a ballot
// and a handful of scalar instructions, no LDS access.  The search starts at the lowest block that
// still has a bin with room.  Every loop is
// bounded by rows * ceil(bins / 64); there are no atomics and nothing to spin on, so the result is
// deterministic.  bin_rows_kernel then moves the rows (a wave per row) and fills each bin's tail:
// every output cell is written exactly once, nothing is memset first.
//
// A length below 0 counts as 0 and one above W as W: no row is read past its end.  A placed row has
// row_start + n <= seq_len and row_bin < bins by construction, so every store is inside its output.
#include <hip/hip_runtime.h>

#include "collate.h"

#include <algorithm>
#include <string>

namespace tkh {

namespace {

constexpr int kBinThreads = 256;
constexpr int kBinWave = 64;
constexpr int kBinRows = kBinThreads / kBinWave;  // rows per workgroup of bin_rows_kernel, one wave each
constexpr int kBinChunk = 4096;                   // cells of one tail-fill task

__device__ __forceinline__ int uniform_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__global__ __launch_bounds__(kBinThreads) void bin_plan_kernel(const int64_t* __restrict__ lengths, int rows, int64_t W,
                                                                int seq_len, int bins, int32_t* __restrict__ row_bin,
                                                                int32_t* __restrict__ row_start,
                                                                int32_t* __restrict__ row_lens,
                                                                int32_t* __restrict__ bin_lens,
                                                                int32_t* __restrict__ n_bins,
                                                                int32_t* __restrict__ unplaced,
                                                                int64_t* __restrict__ cut) {
  __shared__ int room[kBinMaxRows];  // free[]: 64 KiB, the whole LDS a workgroup may declare statically
  const int t = int(threadIdx.x), lane = t & (kBinWave - 1);
  for (int b = t; b < bins; b += kBinThreads) room[b] = seq_len;
  __syncthreads();
  if (t < kBinWave) {
    int low = 0;        // the lowest 64-bin block that may still have a bin with room
    int used = 0;       // one past the highest bin holding an element
    int missed = 0;     // rows that found no bin
    long long lost = 0; // this lane's rows: elements cut off at seq_len
    // room[held + lane] lives in `f` while block `held` is the one being tested: LDS has it again
    // when the search moves to another block (hold) and after the last row
    int held = 0;
    int f = lane < bins ? room[lane] : -1;
    auto hold = [&](int base) {
      if (held + lane < bins) room[held + lane] = f;
      held = base;
      f = base + lane < bins ? room[base + lane] : -1;
    };
    for (int r0 = 0; r0 < rows; r0 += kBinWave) {
      const int r = r0 + lane;
      long long m = 0;
      if (r < rows) {
        const int64_t raw = lengths[r];
        m = raw < 0 ? 0 : (raw > W ? W : raw);
      }
      const int n = int(m < seq_len ? m : seq_len);
      lost += m - n;
      int my_bin = -1, my_start = -1;
      const int count = rows - r0 < kBinWave ? rows - r0 : kBinWave;
      for (int k = 0; k < count; ++k) {
        const int want = uniform_lane(n, k);
        int found = -1, before = 0;
        // the common case first: the block in registers is where the search starts, and the row fits it
        unsigned long long fits = want != 0 && held == low ? __ballot(f >= want) : 0;
        if (fits == 0) {
          if (want == 0) {  // fits the lowest bin whatever it holds
            if (bins > 0) {
              found = 0;
              before = uniform_lane(held == 0 ? f : room[0], 0);
            }
          } else {
            for (int base = low; base < bins; base += kBinWave) {
              if (base != held) hold(base);
              fits = __ballot(f >= want);
              if (fits != 0) break;
              if (base == low && __ballot(f > 0) == 0) low = base + kBinWave;  // the whole block is full
            }
          }
        }
        if (fits != 0) {
          const int src = __builtin_ctzll(fits);
          found = held + src;
          before = uniform_lane(f, src);
          if (lane == src) f -= want;
          used = found + 1 > used ? found + 1 : used;
        }
        missed += found < 0;
        if (lane == k) {
          my_bin = found;
          my_start = found < 0 ? -1 : seq_len - before;
        }
      }
      if (r < rows) {
        row_bin[r] = my_bin;
        row_start[r] = my_start;
        row_lens[r] = n;
      }
    }
    if (held + lane < bins) room[held + lane] = f;
#pragma unroll
    for (int o = kBinWave / 2; o > 0; o >>= 1) lost += __shfl_down(lost, o, kBinWave);
    if (lane == 0) {
      *n_bins = used;
      *unplaced = missed;
      *cut = lost;
    }
  }
  __syncthreads();
  for (int b = t; b < bins; b += kBinThreads) bin_lens[b] = seq_len - room[b];
}

template <typename T>
__global__ __launch_bounds__(kBinThreads) void bin_rows_kernel(const T* __restrict__ padded, int rows, int64_t W,
                                                                int seq_len, int bins,
                                                                const int32_t* __restrict__ row_bin,
                                                                const int32_t* __restrict__ row_start,
                                                                const int32_t* __restrict__ row_lens,
                                                                const int32_t* __restrict__ bin_lens,
                                                                T* __restrict__ values, T pad,
                                                                int32_t* __restrict__ seg, int32_t* __restrict__ pos) {
  const int t = int(threadIdx.x), lane = t & (kBinWave - 1);
  const long long wave = (long long)blockIdx.x * kBinRows + t / kBinWave;
  const long long waves = (long long)gridDim.x * kBinRows;
  for (long long r = wave; r < rows; r += waves) {
    const int b = row_bin[r];
    if (b < 0) continue;  // unplaced: writes nothing
    const int n = row_lens[r];
    const T* __restrict__ src = padded + r * W;
    const long long at = (long long)b * seq_len + row_start[r];
    for (long long i = lane; i < n; i += kBinWave) {
      values[at + i] = src[i];
      seg[at + i] = int32_t(r);
      pos[at + i] = int32_t(i);
    }
  }
  // the tails [bin_lens[b], seq_len), in tasks of kBinChunk cells so that one long tail is shared
  const int chunks = (seq_len + kBinChunk - 1) / kBinChunk;
  const long long tasks = (long long)bins * chunks;
  for (long long task = wave; task < tasks; task += waves) {
    const int b = int(task / chunks), c = int(task % chunks);
    const int filled = bin_lens[b];
    const int lo = filled > c * kBinChunk ? filled : c * kBinChunk;
    const long long hi = std::min<long long>(seq_len, (long long)(c + 1) * kBinChunk);
    const long long at = (long long)b * seq_len;
    for (long long i = (long long)lo + lane; i < hi; i += kBinWave) {
      values[at + i] = pad;
      seg[at + i] = -1;
      pos[at + i] = 0;
    }
  }
}

template <typename T>
void launch_bin_t(const void* padded, int64_t rows, int64_t W, int64_t seq_len, int64_t bins,
                  const int32_t* row_bin, const int32_t* row_start, const int32_t* row_lens, const int32_t* bin_lens,
                  void* values, uint64_t pad_bits, int32_t* seg, int32_t* pos, hipStream_t stream) {
  const int64_t chunks = (seq_len + kBinChunk - 1) / kBinChunk;
  const int64_t work = std::max(rows, std::min<int64_t>(bins * chunks, 4096));  // a wave per row, tails strided
  const dim3 grid(unsigned(std::max<int64_t>(1, (work + kBinRows - 1) / kBinRows)));
  hipLaunchKernelGGL((bin_rows_kernel<T>), grid, dim3(kBinThreads), 0, stream, static_cast<const T*>(padded),
                     int(rows), W, int(seq_len), int(bins), row_bin, row_start, row_lens, bin_lens,
                     static_cast<T*>(values), T(pad_bits), seg, pos);
}

}  // namespace

void launch_bin_rows(const void* padded, int elem_size, int64_t rows, int64_t W, const int64_t* lengths,
                     int64_t seq_len, int64_t bins, void* values, uint64_t pad_bits, int32_t* seg, int32_t* pos,
                     int32_t* bin_lens, int32_t* row_bin, int32_t* row_start, int32_t* row_lens, int32_t* n_bins,
                     int32_t* unplaced, int64_t* cut, hipStream_t stream) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (rows < 0 || W < 0 || bins < 0) throw std::invalid_argument("bin rows: negative rows, width or bins");
  if (seq_len < 1) throw std::invalid_argument("bin rows: seq_len must be at least 1");
  if (rows > kBinMaxRows || bins > kBinMaxRows)
    throw std::invalid_argument("bin rows: rows and bins must not exceed " + std::to_string(kBinMaxRows));
  if (W >= kLimit || seq_len >= kLimit || rows * W >= kLimit || bins * seq_len >= kLimit)
    throw std::invalid_argument("bin rows: rows * width and bins * seq_len must be below 2^31");
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)
    throw std::invalid_argument("bin rows: element size must be 1, 2, 4 or 8 bytes");
  if (n_bins == nullptr || unplaced == nullptr || cut == nullptr)
    throw std::invalid_argument("bin rows: n_bins, unplaced and cut are required");
  if ((rows > 0 && (lengths == nullptr || row_bin == nullptr || row_start == nullptr || row_lens == nullptr)) ||
      (rows * W > 0 && padded == nullptr) || (bins > 0 && (bin_lens == nullptr || values == nullptr ||
                                                            seg == nullptr || pos == nullptr)))
    throw std::invalid_argument("bin rows: null input or output");
  hipLaunchKernelGGL(bin_plan_kernel, dim3(1), dim3(kBinThreads), 0, stream, lengths, int(rows), W, int(seq_len),
                     int(bins), row_bin, row_start, row_lens, bin_lens, n_bins, unplaced, cut);
  switch (elem_size) {
    case 1: launch_bin_t<uint8_t>(padded, rows, W, seq_len, bins, row_bin, row_start, row_lens, bin_lens, values, pad_bits, seg, pos, stream); break;
    case 2: launch_bin_t<uint16_t>(padded, rows, W, seq_len, bins, row_bin, row_start, row_lens, bin_lens, values, pad_bits, seg, pos, stream); break;
    case 4: launch_bin_t<uint32_t>(padded, rows, W, seq_len, bins, row_bin, row_start, row_lens, bin_lens, values, pad_bits, seg, pos, stream); break;
    default: launch_bin_t<uint64_t>(padded, rows, W, seq_len, bins, row_bin, row_start, row_lens, bin_lens, values, pad_bits, seg, pos, stream); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("bin rows launch: ") + hipGetErrorString(e));
}

}  // namespace tkh
