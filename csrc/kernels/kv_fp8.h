// fp8 (OCP e4m3fn) KV cache: the one definition of the row quantization every writer uses and the exact
// in-register dequantization every reader uses (ops/fp8.py quantize_rows is the host form).
//
// A cached row x (one token, one KV head, D bf16 values) is stored as D bytes + one fp32 scale:
//   s = amax|x| * fp32(1/448) (1.0 for an all-zero row), inv = 1/s correctly rounded,
//   x8 = e4m3_rne(x * inv), x ~= x8 * s.
// Readers never touch the 8-bit values with the scale: fp8 -> bf16 is exact (v_cvt_pk_f32_fp8 + v_perm),
// and the per-key scales fold into the fp32 softmax of the attention kernels.
#pragma once
#include "common.h"

namespace ragk {

constexpr float KV8_MAX = 448.f;

__device__ __forceinline__ unsigned kv8_pack4(float a, float b, float c, float d) {
  int v = 0;
  v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
  v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  return (unsigned)v;
}

__device__ __forceinline__ uint2 kv8_quant8(const float* f, float inv) {
  uint2 o;
  o.x = kv8_pack4(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
  o.y = kv8_pack4(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
  return o;
}

__device__ __forceinline__ unsigned kv8_pair_bf16x2(f32x2 f) {
  return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
}

// 8 fp8 (two dwords) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 kv8_to_bf16(unsigned lo, unsigned hi) {
  u32x4 r;
  r[0] = kv8_pair_bf16x2(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false));
  r[1] = kv8_pair_bf16x2(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true));
  r[2] = kv8_pair_bf16x2(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false));
  r[3] = kv8_pair_bf16x2(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true));
  return __builtin_bit_cast(bf16x8, r);
}

// Quantize and store one cache row of D = 128 held by an aligned group of 8 lanes: lane v of the group has
// the row's bf16 values (as floats) d = 8v + [0, 8) in `a` and d = 64 + 8v + [0, 8) in `b` -- the
// (d, d + D/2) rotate_half pairs of the RoPE writers. All 8 lanes of the group must be active.
__device__ __forceinline__ void kv8_store_row128(const float* a, const float* b, int v, unsigned char* drow,
                                                 float* srow) {
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fmaxf(fabsf(a[e]), fabsf(b[e])));
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
  const float s = amax > 0.f ? amax * (1.f / KV8_MAX) : 1.f;
  const float inv = __fdiv_rn(1.f, s);
  *reinterpret_cast<uint2*>(drow + 8 * v) = kv8_quant8(a, inv);
  *reinterpret_cast<uint2*>(drow + 64 + 8 * v) = kv8_quant8(b, inv);
  if (v == 0) *srow = s;
}

}  // namespace ragk
