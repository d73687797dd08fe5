// f32 / bf16 / f16 -> OCP MX block-scaled mxfp8 (e4m3fn) or mxfp4 (e2m1) with E8M0 scales, on gfx950.
//
//   a block = 32 consecutive elements of a contiguous tensor; n_blocks = numel / 32
//   scales[b]                     one E8M0 byte per block (0xFF: the block held a NaN or an infinity)
//   values[32 b .. 32 b + 32)     mxfp8: one e4m3fn byte per element
//   values[16 b .. 16 b + 16)     mxfp4: two e2m1 codes per byte, element 2i in the low nibble
//
// The per-block rules are in mx_block.h (exact; the tests compare bytes).  Memory-bound and
// elementwise with a short reduction: no LDS, no atomics, one launch.
//
// A lane owns kEpl consecutive elements and a block is owned by kLpb = 32 / kEpl adjacent lanes of one
// wave: 8 lanes x 4 elements for f32 -> mxfp8 (a 16-byte load, a dword store per lane), 4 lanes x 8
// elements otherwise (one 16-byte load of bf16 / f16 or two of f32; a dword store for mxfp4, two
// dwords for mxfp8).  The block's amax is the unsigned max of (bits & 0x7fffffff) over its lanes:
// log2(kLpb) xor-shuffles inside the lane group.  Lane 0 of the group stores the scale byte.  Lane
// groups stride over the blocks; a group leaves the loop as a whole, so the shuffles of the groups
// still in it only read lanes that are active.
#include <hip/hip_runtime.h>

#include "collate.h"
#include "mx_block.h"

#include <algorithm>
#include <string>

namespace tkh {

namespace {

constexpr int kMxThreads = 256;

// kN elements at p (16-byte aligned) -> f32, exactly
template <int kN>
__device__ __forceinline__ void mx_load(const float* __restrict__ p, float (&v)[kN]) {
#pragma unroll
  for (int q = 0; q < kN / 4; ++q) {
    const float4 x = reinterpret_cast<const float4*>(p)[q];
    v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
  }
}

__device__ __forceinline__ void mx_load(const __bf16* __restrict__ p, float (&v)[8]) {
  const uint4 x = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[2 * q] = __builtin_bit_cast(float, w[q] << 16);
    v[2 * q + 1] = __builtin_bit_cast(float, w[q] & 0xffff0000u);
  }
}

__device__ __forceinline__ void mx_load(const _Float16* __restrict__ p, float (&v)[8]) {
  typedef _Float16 half8 __attribute__((ext_vector_type(8)));
  const half8 x = *reinterpret_cast<const half8*>(p);
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = float(x[q]);
}

template <typename S, int kFmt>
__global__ __launch_bounds__(kMxThreads) void mx_quant_kernel(const S* __restrict__ src, int64_t n_blocks,
                                                               uint8_t* __restrict__ values,
                                                               uint8_t* __restrict__ scales) {
  constexpr int kEpl = (sizeof(S) == 4 && kFmt == kMxFp8) ? 4 : 8;  // elements per lane
  constexpr int kLpb = kMxBlock / kEpl;                             // lanes per block
  const int64_t groups = int64_t(gridDim.x) * (kMxThreads / kLpb);
  const int j = int(threadIdx.x) % kLpb;
  for (int64_t b = (int64_t(blockIdx.x) * kMxThreads + threadIdx.x) / kLpb; b < n_blocks; b += groups) {
    float v[kEpl];
    mx_load(src + b * kMxBlock + j * kEpl, v);
    uint32_t amax = 0;
#pragma unroll
    for (int e = 0; e < kEpl; ++e) amax = max(amax, __builtin_bit_cast(uint32_t, v[e]) & kMxAbsMask);
#pragma unroll
    for (int o = 1; o < kLpb; o <<= 1) amax = max(amax, uint32_t(__shfl_xor(int(amax), o)));
    const bool bad = mx_bad(amax);
    const int se = mx_scale_exp<kFmt>(amax);
    uint32_t w[kEpl / 4] = {};  // mxfp8: a byte per element; mxfp4: only w[0] is used, a nibble per element
    if (!bad) {
#pragma unroll
      for (int e = 0; e < kEpl; ++e) {
        const uint32_t c = mx_encode<kFmt>(v[e], se);
        if constexpr (kFmt == kMxFp8) w[e / 4] |= c << (8 * (e % 4));
        else w[0] |= c << (4 * e);
      }
    }
    if constexpr (kFmt == kMxFp4) {
      reinterpret_cast<uint32_t*>(values + b * (kMxBlock / 2))[j] = w[0];
    } else if constexpr (kEpl == 4) {
      reinterpret_cast<uint32_t*>(values + b * kMxBlock)[j] = w[0];
    } else {
      reinterpret_cast<uint2*>(values + b * kMxBlock)[j] = make_uint2(w[0], w[1]);
    }
    if (j == 0) scales[b] = bad ? kMxScaleNaN : mx_scale_byte(se);
  }
}

template <typename S, int kFmt>
void launch_mx_t(const void* src, int64_t n_blocks, uint8_t* values, uint8_t* scales, hipStream_t stream) {
  constexpr int kEpl = (sizeof(S) == 4 && kFmt == kMxFp8) ? 4 : 8;
  constexpr int kGroupsPerWg = kMxThreads / (kMxBlock / kEpl);  // 32 (f32 -> mxfp8) or 64 blocks per pass
  // One lane group per block up to kMxMaxGrid workgroups (eight 256-thread workgroups for each of the
  // 256 CUs), the grid-stride loop beyond: with 64 blocks per workgroup that is above 131072 blocks.
  // tests/test_gpu_mx.py runs 131072 + 65 blocks (4 196 384 elements) so that every instantiation
  // takes the loop a second time, the last pass with a partial wave.
  const int64_t wgs = std::min<int64_t>(kMxMaxGrid, (n_blocks + kGroupsPerWg - 1) / kGroupsPerWg);
  hipLaunchKernelGGL((mx_quant_kernel<S, kFmt>), dim3(unsigned(wgs)), dim3(kMxThreads), 0, stream,
                     static_cast<const S*>(src), n_blocks, values, scales);
}

template <int kFmt>
void launch_mx_f(const void* src, int src_dt, int64_t n_blocks, uint8_t* values, uint8_t* scales, hipStream_t stream) {
  switch (src_dt) {
    case kF32: launch_mx_t<float, kFmt>(src, n_blocks, values, scales, stream); break;
    case kBF16: launch_mx_t<__bf16, kFmt>(src, n_blocks, values, scales, stream); break;
    case kF16: launch_mx_t<_Float16, kFmt>(src, n_blocks, values, scales, stream); break;
    default: throw std::invalid_argument("mx quantize: the source must be float32, bfloat16 or float16");
  }
}

}  // namespace

void launch_mx_quantize(const void* src, int src_dt, int64_t n_blocks, int fmt, void* values, uint8_t* scales,
                        hipStream_t stream) {
  if (n_blocks < 0 || n_blocks >= (int64_t(1) << 31) / kMxBlock)
    throw std::invalid_argument("mx quantize: the element count must be in [0, 2^31)");
  if (fmt != kMxFp8 && fmt != kMxFp4) throw std::invalid_argument("mx quantize: format must be 0 (mxfp8) or 1 (mxfp4)");
  if (src_dt != kF32 && src_dt != kBF16 && src_dt != kF16)
    throw std::invalid_argument("mx quantize: the source must be float32, bfloat16 or float16");
  if (n_blocks == 0) return;
  if (src == nullptr || values == nullptr || scales == nullptr)
    throw std::invalid_argument("mx quantize: null input or output");
  if (reinterpret_cast<uintptr_t>(src) % 16 != 0 || reinterpret_cast<uintptr_t>(values) % 16 != 0)
    throw std::invalid_argument("mx quantize: the source and the values must be 16-byte aligned");
  uint8_t* dst = static_cast<uint8_t*>(values);
  if (fmt == kMxFp8) launch_mx_f<kMxFp8>(src, src_dt, n_blocks, dst, scales, stream);
  else launch_mx_f<kMxFp4>(src, src_dt, n_blocks, dst, scales, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("mx quantize launch: ") + hipGetErrorString(e));
}

}  // namespace tkh
