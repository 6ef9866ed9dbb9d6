// 4-bit integer weight GEMM for gfx950 (AWQ / GPTQ checkpoints; ops/int4.py). 4.25 bits per weight:
//   W[n][k] = fp16 scale[n][k/128] * (code[n][k] - zero[n][k/128]), code 0..15, zero 0..16
//   meta  int32 [rows, K/128]: bits 0..15 the fp16 scale, bits 16..20 the zero point
//   packed uint8 [rows, K/2]: of each 8 consecutive k (one dword d), byte j holds code k0+j in its low nibble
//          and code k0+4+j in its high nibble: d & 0x0f0f0f0f = codes k0..k0+3 and (d >> 4) & 0x0f0f0f0f =
//          codes k0+4..k0+7, one per byte, in k order.
//
//  * gemm_int4_dec : decode (M <= 64), W4A16. One 16-column tile per workgroup, 8 waves take interleaved
//                    128-deep K blocks, per lane and K block one 16-byte non-temporal weight load (k = 32 fh ..
//                    32 fh + 31 of the lane's row) and one meta dword, the next block's pair in flight while this
//                    one is converted (the conversion below is ~5x the VALU work of the MXFP4 kernel's, so a wave
//                    cannot count on its neighbours alone to cover the load).
//                    gfx950 has no packed bf16 arithmetic (v_pk_add_bf16 and kin do not assemble), so the
//                    "OR the nibble into the mantissa of 128.0, subtract 128 + zero" route would go through fp32
//                    per element anyway. Instead: the byte-per-code layout above, v_cvt_f32_ubyte{0..3} (code ->
//                    fp32, one per weight), v_pk_add_f32 with -zero and v_cvt_pk_bf16_f32 (both one per pair):
//                    19 VALU per 8 weights against about 23 for the mantissa route. code - zero is an integer of
//                    magnitude <= 16: exact in bf16, no weight is ever rounded.
//                    The four MFMAs of a K block start from a zero accumulator and the block is folded in as
//                    acc = fma(fp32(scale), part, acc): in the 16x16x32 layout the accumulator's column is
//                    lane & 15, the weight row whose bytes and meta word this lane loaded, so the scale is
//                    already in the right lane. Partials meet in LDS and are summed in wave order: no atomics,
//                    two launches give the same bits.
//                    The split is the decode family's (gemm_fp8_dec, gemm_mxfp4_dec). Cutting a K block between
//                    waves would even out counts like 9 blocks over 8 waves, but a lane's 16-byte load is one
//                    quarter of a block and the scale fold wants whole blocks; the served shapes (K = 4096,
//                    8192, 14336, 28672) are multiples of 8 blocks, so the interleaved split stays.
//  * dequant_int4  : Int4Weight -> bf16 [rows, K] at a row pitch, bf16_rne(fp32(scale) * (code - zero)), one
//                    dword in and one 16-byte store out per thread. The M > 64 route runs the bf16 GEMM on it.
#include "common.h"
using namespace ragk;

namespace {

constexpr int DW = 8;  // waves per block, split K

__device__ __forceinline__ float meta_scale(unsigned m) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(m & 0xffffu));
}
__device__ __forceinline__ float meta_zero(unsigned m) { return (float)((m >> 16) & 31u); }

// four codes, one per byte -> fp32 (v_cvt_f32_ubyte0..3)
__device__ __forceinline__ void bytes_to_f32(unsigned b, float* f) {
  f[0] = (float)(b & 0xffu);
  f[1] = (float)((b >> 8) & 0xffu);
  f[2] = (float)((b >> 16) & 0xffu);
  f[3] = (float)(b >> 24);
}

// one dword = 8 codes -> the 8 bf16 integers code - zero in k order (nz = -zero)
__device__ __forceinline__ bf16x8 int4x8_to_bf16(unsigned d, float nz) {
  float f[8];
  bytes_to_f32(d & 0x0f0f0f0fu, f);
  bytes_to_f32((d >> 4) & 0x0f0f0f0fu, f + 4);
  const f32x2 z2 = (f32x2){nz, nz};
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 p = (f32x2){f[2 * i], f[2 * i + 1]} + z2;
    r[i] = pk2bf(p[0], p[1]);
  }
  return __builtin_bit_cast(bf16x8, r);
}

template <int MT, int EPI, bool OUT_F32>
__global__ __launch_bounds__(DW * 64) void gemm_int4_dec_kernel(const bf16_t* __restrict__ X, int ldx,
                                                                const unsigned char* __restrict__ W, int ldw,
                                                                const unsigned* __restrict__ META, int ldm, void* C,
                                                                int ldc, const bf16_t* __restrict__ bias,
                                                                const bf16_t* resid, int ldr, int M, int N, int K) {
  constexpr bool PAIR = (EPI == EPI_SILU_MUL);
  constexpr int NACC = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) f32x4 red[DW][NACC * MT][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int n0 = blockIdx.x * 16;
  int wrow[NACC];
  if constexpr (PAIR) {  // packed [64 gate | 64 up] rows: output column g pairs rows (g / 64) * 128 + g % 64, + 64
    const int g = n0 + fr;
    wrow[0] = (g >> 6) * 128 + (g & 63);
    wrow[1] = wrow[0] + 64;
  } else {
    wrow[0] = min(n0 + fr, N - 1);
  }
  const unsigned char* wp[NACC];
  const unsigned* mp[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    wp[a] = W + (size_t)wrow[a] * ldw + 16 * fh;
    mp[a] = META + (size_t)wrow[a] * ldm;
  }
  const bf16_t* xr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xr[t] = X + (size_t)min(t * 16 + fr, M - 1) * ldx + 32 * fh;

  f32x4 acc[NACC][MT];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[a][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nkb = K >> 7;
  // block b of this lane's rows: 16 weight bytes + the meta word; b clamped, so the prefetch past a wave's last
  // block (and a wave with no block at all) reads valid memory it never uses
  u32x4 cv[NACC], nv[NACC];
  unsigned cm[NACC], nm[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int b = min(wid, nkb - 1);
    cv[a] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[a] + b * 64));
    cm[a] = mp[a][b];
  }
  for (int kb = wid; kb < nkb; kb += DW) {
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      const int b = min(kb + DW, nkb - 1);
      nv[a] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[a] + b * 64));
      nm[a] = mp[a][b];
    }
    bf16x8 xf[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) xf[t][s] = *reinterpret_cast<const bf16x8*>(xr[t] + kb * 128 + 8 * s);
    float nz[NACC];
    f32x4 part[NACC][MT];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      nz[a] = -meta_zero(cm[a]);
#pragma unroll
      for (int t = 0; t < MT; ++t) part[a][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 wf[NACC];
#pragma unroll
      for (int a = 0; a < NACC; ++a) wf[a] = int4x8_to_bf16(cv[a][s], nz[a]);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int a = 0; a < NACC; ++a)
          part[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[t][s], wf[a], part[a][t], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      const float sc = meta_scale(cm[a]);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][t][r] = __builtin_fmaf(sc, part[a][t][r], acc[a][t][r]);
      cv[a] = nv[a];
      cm[a] = nm[a];
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int t = 0; t < MT; ++t) red[wid][a * MT + t][lane] = acc[a][t];
  __syncthreads();

  for (int e = threadIdx.x; e < MT * 64 * 4; e += DW * 64) {
    const int t = e >> 8, ln = (e >> 2) & 63, r = e & 3;
    const int row = t * 16 + 4 * (ln >> 4) + r;
    const int col = n0 + (ln & 15);
    if (row >= M || col >= N) continue;
    float v = 0.f, u = 0.f;
#pragma unroll
    for (int w = 0; w < DW; ++w) {
      v += red[w][t][ln][r];
      if constexpr (PAIR) u += red[w][MT + t][ln][r];
    }
    if constexpr (PAIR) v = silu(v) * u;
    if constexpr (EPI == EPI_BIAS || EPI == EPI_BIAS_RESID || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_TANH)
      v += bf2f(bias[col]);
    if constexpr (EPI == EPI_RESID || EPI == EPI_BIAS_RESID) v += bf2f(resid[(size_t)row * ldr + col]);
    if constexpr (EPI == EPI_BIAS_GELU || EPI == EPI_GELU) v = gelu_erf(v);
    if constexpr (EPI == EPI_BIAS_GELU_TANH) v = gelu_tanh(v);
    if constexpr (OUT_F32)
      reinterpret_cast<float*>(C)[(size_t)row * ldc + col] = v;
    else
      reinterpret_cast<bf16_t*>(C)[(size_t)row * ldc + col] = f2bf(v);
  }
}

// one thread: 8 codes (one dword) -> 8 bf16 (one 16-byte store)
__global__ __launch_bounds__(256) void dequant_int4_kernel(const unsigned char* __restrict__ W, int ldw,
                                                           const unsigned* __restrict__ META, int ldm,
                                                           bf16_t* __restrict__ out, int ldo, int rows, int K) {
  const int dpr = K >> 3;  // dwords per row
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * dpr) return;
  const int row = (int)(idx / dpr), c = (int)(idx % dpr);
  const unsigned d = *reinterpret_cast<const unsigned*>(W + (size_t)row * ldw + 4 * c);
  const unsigned m = META[(size_t)row * ldm + (c >> 4)];
  const float sc = meta_scale(m), z = meta_zero(m);
  float f[8];
  bytes_to_f32(d & 0x0f0f0f0fu, f);
  bytes_to_f32((d >> 4) & 0x0f0f0f0fu, f + 4);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = sc * (f[e] - z);
  *reinterpret_cast<u32x4*>(out + (size_t)row * ldo + 8 * c) = pack8(f);
}

template <int MT, int EPI, bool F32>
hipError_t launch_dec(const void* X, int ldx, const void* W, int ldw, const void* MW, int ldm, void* C, int ldc,
                      const void* bias, const void* resid, int ldr, int M, int N, int K, hipStream_t st) {
  hipLaunchKernelGGL((gemm_int4_dec_kernel<MT, EPI, F32>), dim3((N + 15) / 16), dim3(DW * 64), 0, st,
                     (const bf16_t*)X, ldx, (const unsigned char*)W, ldw, (const unsigned*)MW, ldm, C, ldc,
                     (const bf16_t*)bias, (const bf16_t*)resid, ldr, M, N, K);
  return hipGetLastError();
}

template <int EPI, bool F32>
hipError_t dispatch_dec(const void* X, int ldx, const void* W, int ldw, const void* MW, int ldm, void* C, int ldc,
                        const void* bias, const void* resid, int ldr, int M, int N, int K, hipStream_t st) {
  switch ((M + 15) / 16) {
    case 1: return launch_dec<1, EPI, F32>(X, ldx, W, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
    case 2: return launch_dec<2, EPI, F32>(X, ldx, W, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
    case 3: return launch_dec<3, EPI, F32>(X, ldx, W, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
    case 4: return launch_dec<4, EPI, F32>(X, ldx, W, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
    default: return hipErrorInvalidValue;
  }
}

// packed rows of 16-byte lane loads, one meta word per row and 128 k
bool int4_layout_ok(const void* W4, int ldw, const void* MW, int ldm, int K) {
  return K % 128 == 0 && ldw % 16 == 0 && ldw >= K / 2 && (size_t)W4 % 16 == 0 && ldm >= K / 128 && (size_t)MW % 4 == 0;
}

}  // namespace

// Decode W4A16 (M <= 64): C = epi(x . dequant(W4, MW)^T). x bf16 [M, K] (row stride ldx elements, 16-byte
// aligned rows), W4 [N or 2N, K/2] packed codes (row stride ldw bytes), MW [N or 2N, K/128] meta words (row
// stride ldm words). N = output columns; for EPI_SILU_MUL the weight has 2N rows in the packed
// [64 gate | 64 up] tile layout.
RAGK_API int ragk_gemm_int4(const void* x, int ldx, const void* W4, int ldw, const void* MW, int ldm, void* C, int ldc,
                            const void* bias, const void* resid, int ldr, int M, int N, int K, int epi, int out_f32,
                            hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (!int4_layout_ok(W4, ldw, MW, ldm, K) || M > 64 || (size_t)x % 16 || (M > 1 && (ldx % 8 || ldx < K)))
    return (int)hipErrorInvalidValue;
  if (epi == EPI_SILU_MUL) {
    if (N % 64 || out_f32) return (int)hipErrorInvalidValue;
    return (int)dispatch_dec<EPI_SILU_MUL, false>(x, ldx, W4, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
  }
#define RAGK_INT4_CASE(E)                                                                                          \
  case E:                                                                                                          \
    return out_f32 ? (int)dispatch_dec<E, true>(x, ldx, W4, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st)   \
                   : (int)dispatch_dec<E, false>(x, ldx, W4, ldw, MW, ldm, C, ldc, bias, resid, ldr, M, N, K, st);
  switch (epi) {
    RAGK_INT4_CASE(EPI_NONE)
    RAGK_INT4_CASE(EPI_BIAS)
    RAGK_INT4_CASE(EPI_RESID)
    RAGK_INT4_CASE(EPI_BIAS_RESID)
    RAGK_INT4_CASE(EPI_BIAS_GELU)
    RAGK_INT4_CASE(EPI_GELU)
    RAGK_INT4_CASE(EPI_BIAS_GELU_TANH)
    default: return (int)hipErrorInvalidValue;
  }
#undef RAGK_INT4_CASE
}

// out[rows, K] bf16 (row stride ldo elements, 16-byte aligned rows) = bf16_rne(fp32(scale) * (code - zero))
RAGK_API int ragk_dequant_int4(const void* W4, int ldw, const void* MW, int ldm, void* out, int ldo, int rows, int K,
                               hipStream_t st) {
  if (rows <= 0 || K <= 0) return 0;
  if (!int4_layout_ok(W4, ldw, MW, ldm, K) || ldo % 8 || ldo < K || (size_t)out % 16) return (int)hipErrorInvalidValue;
  const size_t threads = (size_t)rows * (K / 8);
  if (threads > (size_t)0x7fffffff * 256) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dequant_int4_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                     (const unsigned char*)W4, ldw, (const unsigned*)MW, ldm, (bf16_t*)out, ldo, rows, K);
  return (int)hipGetLastError();
}
