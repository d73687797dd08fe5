// The per-block math of OCP Microscaling (MX v1.0) quantisation, shared by the gfx950 kernel
// (mx_quant.hip) and by host programs that rehearse it: a block is 32 consecutive f32 values, its
// scale one E8M0 byte, its elements e4m3fn (mxfp8) or e2m1 (mxfp4).  Everything here is exact
// integer / power-of-two arithmetic followed by one round-to-nearest-even.
//
//   amax_bits  max over the block of (bits & 0x7fffffff): an unsigned compare orders |v|, and the one
//              integer gives floor(log2(amax)) (its exponent field), the zero block and `bad`
//              (>= 0x7f800000: the block holds a NaN or an infinity).
//   se         clamp(E - emax, -127, 127), E = (amax_bits >> 23) - 127.  A subnormal or zero amax has
//              exponent field 0, E = -127, which the clamp takes to -127 whatever its true exponent.
//   element    RNE(clamp(ldexp(v, -se), -top, +top)); the clamp is the MX saturation (a plain e4m3fn
//              cast turns 465..511 into NaN).  The sign of v is kept, so -0.0 stays a negative zero.
//   bad block  scale byte 0xFF (E8M0 NaN), every element byte 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dtypes.h"

namespace tkh {

enum MxFormat : int { kMxFp8 = 0, kMxFp4 = 1 };

constexpr int kMxBlock = 32;
constexpr uint32_t kMxAbsMask = 0x7fffffffu;
constexpr uint32_t kMxInfBits = 0x7f800000u;
constexpr uint8_t kMxScaleNaN = 0xFF;

template <int kFmt> struct MxElem;
template <> struct MxElem<kMxFp8> {
  static constexpr int emax = 8;
  static constexpr float top = 448.0f;
};
template <> struct MxElem<kMxFp4> {
  static constexpr int emax = 2;
  static constexpr float top = 6.0f;
};

__host__ __device__ __forceinline__ bool mx_bad(uint32_t amax_bits) { return amax_bits >= kMxInfBits; }

// the block's scale exponent, for a block that is not bad: in [-127, 125]
template <int kFmt>
__host__ __device__ __forceinline__ int mx_scale_exp(uint32_t amax_bits) {
  const int se = int(amax_bits >> 23) - 127 - MxElem<kFmt>::emax;
  return se < -127 ? -127 : se;
}

__host__ __device__ __forceinline__ uint8_t mx_scale_byte(int se) { return uint8_t(se + 127); }

// v / 2^se, exactly (v_ldexp_f32 on the device), saturated to the element format's range
template <int kFmt>
__host__ __device__ __forceinline__ float mx_scaled(float v, int se) {
  const float y = ldexpf(v, -se);
  constexpr float top = MxElem<kFmt>::top;
  return y < -top ? -top : (y > top ? top : y);  // no NaN reaches this; -0.0 passes through
}

// |y| <= 6 -> e2m1 code (sign << 3 | index into 0, .5, 1, 1.5, 2, 3, 4, 6), round to nearest, the
// midpoints .25, .75, 1.25, 1.75, 2.5, 3.5 and 5 to the even index
__host__ __device__ __forceinline__ uint32_t f32_to_e2m1(float y) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, y);
  const float a = __builtin_bit_cast(float, bits & kMxAbsMask);
  const uint32_t idx = uint32_t(a > 0.25f) + uint32_t(a >= 0.75f) + uint32_t(a > 1.25f) + uint32_t(a >= 1.75f) +
                       uint32_t(a > 2.5f) + uint32_t(a >= 3.5f) + uint32_t(a > 5.0f);
  return ((bits >> 28) & 8u) | idx;
}

// One element of a block that is not bad -> its byte (mxfp8) or 4-bit code (mxfp4).
template <int kFmt>
__host__ __device__ __forceinline__ uint32_t mx_encode(float v, int se) {
  const float y = mx_scaled<kFmt>(v, se);
  if constexpr (kFmt == kMxFp8) return f32_to_fp8e4m3fn(y);
  else return f32_to_e2m1(y);
}

}  // namespace tkh
