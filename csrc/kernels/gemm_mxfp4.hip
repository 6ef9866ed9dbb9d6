// OCP MXFP4 weight GEMMs for gfx950: e2m1 weights, two per byte (element k in the low nibble of
// byte k/2 when k is even), one E8M0 scale byte per row and per 32 consecutive k
// (W[n][k] = LUT[code] * 2^(scale[n][k/32] - 127); ops/mxfp4.py). 4.25 bits per weight.
//
//  * gemm_mxfp4_dec : decode (M <= 64), W4A16. The gemm_fp8_dec decomposition -- 8 waves split K
//                     over one 16-column tile, LDS reduction -- with the weights streamed at half a
//                     byte each. Inside a 128-deep K block lane group fh owns k in [32 fh, 32 fh + 32):
//                     exactly one MX block, i.e. one 16-B weight load and one scale byte per lane.
//                     v_cvt_scalef32_pk_bf16_fp4 turns a byte (two e2m1) times the power-of-two block
//                     scale into two bf16 -- exact -- and the product is the bf16 MFMA against the
//                     unquantized activations. The only error is fp32 summation order.
//  * gemm_mxfp4_tile: prefill (M > 64), W4A8. Activations quantized per token by quant_rows
//                     (gemm_fp8.hip); 128x128 tile, LDS-DMA staging as gemm_fp8_tile, and
//                     v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (unit scale) and B = e2m1 with the
//                     weight's own E8M0 block scales, so the epilogue scales by sa[m] only. A B-tile
//                     row is 64 bytes per K step: 16 rows x 4 chunks per 1-KiB LDS-DMA.
//
// Operand layout of the scaled MFMA (pinned bit-exactly by tests/test_mxfp4_gpu.py): for the e2m1
// operand lane (fr, fh) holds row fr, k = 32 fh + j, j = 0..31 in nibble order, in the low 4 dwords
// of the 8-dword vector, and the scale byte that lane selects applies to its own row and its own
// 32-element block. The e4m3 operand is laid out differently: its 8 dwords are two halves, k = 16 fh + j
// and k = 64 + 16 fh + j, j = 0..15 (gemm_fp8_tile never sees this, both its operands being 8-bit).
#include "common.h"
using namespace ragk;

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte load from a 4-byte aligned address

namespace {

// E8M0 byte (1..254) -> the fp32 value 2^(byte - 127): the byte is the fp32 exponent field
__device__ __forceinline__ float e8m0_to_f32(unsigned b) { return __uint_as_float(b << 23); }

// ----------------------------------------------------------------------------- prefill tile
constexpr int BM = 128, BN = 128;
constexpr int BKA = 128;  // A bytes (e4m3 elements) per K step
constexpr int BKW = 64;   // B bytes (two e2m1 each) per K step
constexpr int TILE_THREADS = 256;
constexpr int STAGE_BYTES = BM * BKA + BN * BKW;
constexpr int EPI_LD = BN + 4;
constexpr int EPI_BYTES = BM * EPI_LD * 4;
constexpr int TILE_LDS = (2 * STAGE_BYTES > EPI_BYTES) ? 2 * STAGE_BYTES : EPI_BYTES;
constexpr int GROUP_M = 8;

// A: 128-B rows, 8 chunks of 16 B (as gemm_fp8_tile). B: 64-B rows, 4 chunks; four rows share one
// 256-B bank row, so the swizzle turns with row / 4 and 16 consecutive rows of one chunk column
// cover all 16 bank groups.
__device__ __forceinline__ int swz_a(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int swz_b(int row, int chunk) { return chunk ^ ((row >> 2) & 3); }

__device__ __forceinline__ void stage_a(const unsigned char* __restrict__ g, int ld, int row0, int rows_valid, int k0,
                                        char* lds_tile, int wid, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = wid * 4 + i;
    const int r = q * 8 + (lane >> 3);
    const int c = swz_a(r, lane & 7);
    int gr = row0 + r;
    gr = gr < rows_valid ? gr : rows_valid - 1;
    glds16(g + (size_t)gr * ld + k0 + c * 16, lds_tile + q * 1024);
  }
}

// k0b: byte offset of the K step inside a packed weight row
__device__ __forceinline__ void stage_b(const unsigned char* __restrict__ g, int ld, int row0, int rows_valid, int k0b,
                                        char* lds_tile, int wid, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = wid * 2 + i;
    const int r = q * 16 + (lane >> 2);
    const int c = swz_b(r, lane & 3);
    int gr = row0 + r;
    gr = gr < rows_valid ? gr : rows_valid - 1;
    glds16(g + (size_t)gr * ld + k0b + c * 16, lds_tile + q * 1024);
  }
}

// An 8-bit operand is two 16-byte halves: lane (fr, fh) holds A[row fr][k = 16 fh + j] in dwords 0..3 and
// A[row fr][k = 64 + 16 fh + j] in dwords 4..7, j = 0..15: chunks fh and 4 + fh of the 128-B row
__device__ __forceinline__ i32x8 frag_a(const char* tile, int R, int fh) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + R * 128 + 16 * swz_a(R, fh));
  const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + R * 128 + 16 * swz_a(R, 4 + fh));
  return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// lane (fr, fh) holds B[row fr][k = 32 fh + j] as 32 nibbles: chunk fh of the 64-B row, low 4 dwords
__device__ __forceinline__ i32x8 frag_b(const char* tile, int R, int fh) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + R * 64 + 16 * swz_b(R, fh));
  return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], 0, 0, 0, 0};
}

template <int EPI, bool OUT_F32>
__global__ __launch_bounds__(TILE_THREADS, 2) void gemm_mxfp4_tile_kernel(
    const unsigned char* __restrict__ A, int lda, const float* __restrict__ sa, const unsigned char* __restrict__ B,
    int ldb, const unsigned char* __restrict__ SB, int lds, void* C, int ldc, const bf16_t* __restrict__ bias,
    const bf16_t* resid, int ldr, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char smem[TILE_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  const int logical = xcd_remap(blockIdx.x, nwg);
  const int group = logical / (GROUP_M * tiles_n);
  const int first_m = group * GROUP_M;
  const int gm = min(tiles_m - first_m, GROUP_M);
  const int in_group = logical % (GROUP_M * tiles_n);
  const int tm = first_m + in_group % gm;
  const int tn = in_group / gm;
  const int m0 = tm * BM, n0 = tn * BN;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = K / BKA;
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const int fr = lane & 15, fh = lane >> 4;
  // This lane's scale byte at K step kt: row (n0 + wc*64 + 16 j + fr), block 4 kt + fh, i.e. byte fh of the
  // row's dword kt. A row's dwords are loaded four K steps at a time (one 16-B load per row and group, the next
  // group in flight during the current one): a byte or dword load per K step touches 16 cache lines per
  // instruction, 64 per wave and step against the 48 of the tile's LDS-DMA, and cost a third of the MFMA rate.
  // Group g starts at dword min(4 g, nk - 4), so the last load never runs past the row.
  const unsigned* srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    srow[j] = reinterpret_cast<const unsigned*>(SB + (size_t)min(n0 + wc * 64 + 16 * j + fr, N - 1) * lds);
  u32x4 scur[4], snxt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    snxt[j] = (u32x4){0, 0, 0, 0};
    if (nk >= 4) {
      scur[j] = *reinterpret_cast<const u32x4_a4*>(srow[j]);
    } else {
      scur[j] = (u32x4){srow[j][0], nk > 1 ? srow[j][1] : 0u, nk > 2 ? srow[j][2] : 0u, 0u};
    }
  }

  stage_a(A, lda, m0, M, 0, smem, wid_u, lane);
  stage_b(B, ldb, n0, N, 0, smem + BM * BKA, wid_u, lane);
  wait_vmcnt0();
  __syncthreads();
  // a use of the first scales here, so the compiler retires their loads before the loop: it cannot see the
  // hand-placed wait above, and carried into the loop they become a vmcnt(0) in front of the first MFMA of
  // every K step
  asm volatile("" ::"v"(scur[0]), "v"(scur[1]), "v"(scur[2]), "v"(scur[3]));

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int sg = kt >> 2;
    const int sidx = kt - (nk >= 4 ? min(4 * sg, nk - 4) : 0);  // this step's dword inside scur, 0..3
    int sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned d = sidx == 0 ? scur[j][0] : sidx == 1 ? scur[j][1] : sidx == 2 ? scur[j][2] : scur[j][3];
      sc[j] = (int)(d >> (8 * fh));  // the MFMA takes byte 0 (opsel 0); the upper bytes are ignored
    }
    if (kt + 1 < nk) {
      char* nxt = smem + (cur ^ 1) * STAGE_BYTES;
      stage_a(A, lda, m0, M, (kt + 1) * BKA, nxt, wid_u, lane);
      stage_b(B, ldb, n0, N, (kt + 1) * BKW, nxt + BM * BKA, wid_u, lane);
      if ((kt & 3) == 0 && 4 * (sg + 1) < nk) {
        const int off = min(4 * (sg + 1), nk - 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) snxt[j] = *reinterpret_cast<const u32x4_a4*>(srow[j] + off);
      }
    }
    const char* ta = smem + cur * STAGE_BYTES;
    const char* tb = ta + BM * BKA;
    i32x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = frag_a(ta, wr * 64 + 16 * i + fr, fh);
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = frag_b(tb, wc * 64 + 16 * j + fr, fh);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bfr[j], acc[i][j], 0 /*A e4m3*/,
                                                                     4 /*B e2m1*/, 0, 127, 0, sc[j]);
    // The wait for the next tile's LDS-DMA names the accumulators, so every MFMA of the step is issued in
    // front of it and the DMA flies under them (left alone the compiler sinks the MFMAs below the barrier).
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                   "+v"(acc[1][2]), "+v"(acc[1][3]), "+v"(acc[2][0]), "+v"(acc[2][1]), "+v"(acc[2][2]), "+v"(acc[2][3]),
                   "+v"(acc[3][0]), "+v"(acc[3][1]), "+v"(acc[3][2]), "+v"(acc[3][3])
                 :
                 : "memory");
    __syncthreads();
    if ((kt & 3) == 3) {
      // pinned behind the wait above: moved up as selects, the copy would put a vmcnt(0) among the MFMAs
      asm volatile("" : "+v"(snxt[0]), "+v"(snxt[1]), "+v"(snxt[2]), "+v"(snxt[3]));
#pragma unroll
      for (int j = 0; j < 4; ++j) scur[j] = snxt[j];
    }
  }

  // ---- epilogue: activation row scale -> padded f32 LDS tile -> fused epilogue -> 16-B stores
  float* sC = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wr * 64 + 16 * i + 4 * fh + r;
      const float s = sa[min(m0 + row, M - 1)];
#pragma unroll
      for (int j = 0; j < 4; ++j) sC[row * EPI_LD + wc * 64 + 16 * j + fr] = acc[i][j][r] * s;
    }
  __syncthreads();

  if constexpr (EPI == EPI_SILU_MUL) {
    const int ocol0 = tn * 64;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int v = tid + it * TILE_THREADS;
      const int row = v >> 3, c8 = (v & 7) * 8;
      const int gr = m0 + row;
      if (gr < M) {
        float o[8];
        const float* g = sC + row * EPI_LD + c8;
        const float* u = g + 64;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = silu(g[e]) * u[e];
        *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(C) + (size_t)gr * ldc + ocol0 + c8) = pack8(o);
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int v = tid + it * TILE_THREADS;
      const int row = v >> 4, c8 = (v & 15) * 8;
      const int gr = m0 + row, gc = n0 + c8;
      if (gr < M && gc < N) {
        float o[8];
        const float* s = sC + row * EPI_LD + c8;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = s[e];
        if constexpr (EPI == EPI_BIAS || EPI == EPI_BIAS_RESID || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_TANH) {
          float b[8];
          unpack8(*reinterpret_cast<const u32x4*>(bias + gc), b);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += b[e];
        }
        if constexpr (EPI == EPI_RESID || EPI == EPI_BIAS_RESID) {
          float rr[8];
          unpack8(*reinterpret_cast<const u32x4*>(resid + (size_t)gr * ldr + gc), rr);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += rr[e];
        }
        if constexpr (EPI == EPI_BIAS_GELU || EPI == EPI_GELU) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = gelu_erf(o[e]);
        }
        if constexpr (EPI == EPI_BIAS_GELU_TANH) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = gelu_tanh(o[e]);
        }
        if constexpr (OUT_F32) {
          float* dst = reinterpret_cast<float*>(C) + (size_t)gr * ldc + gc;
          *reinterpret_cast<f32x4*>(dst) = (f32x4){o[0], o[1], o[2], o[3]};
          *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){o[4], o[5], o[6], o[7]};
        } else {
          *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(C) + (size_t)gr * ldc + gc) = pack8(o);
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------- decode
constexpr int DW = 8;  // waves per block, split K

// one dword = 8 e2m1 (k ascending from the low nibble) times `scale` -> 8 bf16, exact:
// one v_cvt_scalef32_pk_bf16_fp4 per byte
__device__ __forceinline__ bf16x8 fp4x8_to_bf16(unsigned w, float scale) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return __builtin_bit_cast(bf16x8, r);
}

// Block = DW waves on one 16-column output tile; waves take interleaved 128-deep K blocks.
// Inside a K block lane group fh owns k in [32 fh, 32 fh + 32): 16 contiguous weight bytes and one
// scale byte; MFMA s consumes k = 32 fh + 8 s + j on both operands.
template <int MT, int EPI, bool OUT_F32>
__global__ __launch_bounds__(DW * 64) void gemm_mxfp4_dec_kernel(const bf16_t* __restrict__ X, int ldx,
                                                                 const unsigned char* __restrict__ W, int ldw,
                                                                 const unsigned char* __restrict__ SW, int lds,
                                                                 void* C, int ldc, const bf16_t* __restrict__ bias,
                                                                 const bf16_t* resid, int ldr, int M, int N, int K) {
  constexpr bool PAIR = (EPI == EPI_SILU_MUL);
  constexpr int NACC = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) f32x4 red[DW][NACC * MT][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int n0 = blockIdx.x * 16;
  int wrow0, wrow1 = 0;
  if constexpr (PAIR) {
    const int g = n0 + fr;
    wrow0 = (g >> 6) * 128 + (g & 63);
    wrow1 = wrow0 + 64;
  } else {
    wrow0 = min(n0 + fr, N - 1);
  }
  const unsigned char* w0 = W + (size_t)wrow0 * ldw + 16 * fh;
  const unsigned char* w1 = W + (size_t)wrow1 * ldw + 16 * fh;
  const unsigned char* s0 = SW + (size_t)wrow0 * lds + fh;
  const unsigned char* s1 = SW + (size_t)wrow1 * lds + fh;
  const bf16_t* xr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xr[t] = X + (size_t)min(t * 16 + fr, M - 1) * ldx + 32 * fh;

  f32x4 acc[NACC][MT];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[a][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nkb = K >> 7;
  for (int kb = wid; kb < nkb; kb += DW) {
    const int k = kb * 128;
    u32x4 wv[NACC];
    float sc[NACC];
    wv[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w0 + kb * 64));
    sc[0] = e8m0_to_f32(s0[kb * 4]);
    if constexpr (PAIR) {
      wv[1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w1 + kb * 64));
      sc[1] = e8m0_to_f32(s1[kb * 4]);
    }
    bf16x8 xf[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) xf[t][s] = *reinterpret_cast<const bf16x8*>(xr[t] + k + 8 * s);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 wf[NACC];
#pragma unroll
      for (int a = 0; a < NACC; ++a) wf[a] = fp4x8_to_bf16(wv[a][s], sc[a]);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int a = 0; a < NACC; ++a)
          acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[t][s], wf[a], acc[a][t], 0, 0, 0);
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

template <int EPI, bool F32>
hipError_t launch_tile4(const void* A, int lda, const float* sa, const void* B, int ldb, const void* SB, int lds,
                        void* C, int ldc, const void* bias, const void* resid, int ldr, int M, int N, int K,
                        hipStream_t st) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  hipLaunchKernelGGL((gemm_mxfp4_tile_kernel<EPI, F32>), dim3(tiles), dim3(TILE_THREADS), 0, st,
                     (const unsigned char*)A, lda, sa, (const unsigned char*)B, ldb, (const unsigned char*)SB, lds, C,
                     ldc, (const bf16_t*)bias, (const bf16_t*)resid, ldr, M, N, K);
  return hipGetLastError();
}

template <int MT, int EPI, bool F32>
hipError_t launch_dec4(const void* X, int ldx, const void* W, int ldw, const void* SW, int lds, void* C, int ldc,
                       const void* bias, const void* resid, int ldr, int M, int N, int K, hipStream_t st) {
  hipLaunchKernelGGL((gemm_mxfp4_dec_kernel<MT, EPI, F32>), dim3((N + 15) / 16), dim3(DW * 64), 0, st,
                     (const bf16_t*)X, ldx, (const unsigned char*)W, ldw, (const unsigned char*)SW, lds, C, ldc,
                     (const bf16_t*)bias, (const bf16_t*)resid, ldr, M, N, K);
  return hipGetLastError();
}

template <int EPI, bool F32>
hipError_t dispatch_dec4(const void* X, int ldx, const void* W, int ldw, const void* SW, int lds, void* C, int ldc,
                         const void* bias, const void* resid, int ldr, int M, int N, int K, hipStream_t st) {
  switch ((M + 15) / 16) {
    case 1: return launch_dec4<1, EPI, F32>(X, ldx, W, ldw, SW, lds, C, ldc, bias, resid, ldr, M, N, K, st);
    case 2: return launch_dec4<2, EPI, F32>(X, ldx, W, ldw, SW, lds, C, ldc, bias, resid, ldr, M, N, K, st);
    case 3: return launch_dec4<3, EPI, F32>(X, ldx, W, ldw, SW, lds, C, ldc, bias, resid, ldr, M, N, K, st);
    case 4: return launch_dec4<4, EPI, F32>(X, ldx, W, ldw, SW, lds, C, ldc, bias, resid, ldr, M, N, K, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

// Prefill W4A8: C = epi((A8 * sa) . dequant(B4, SB)^T); A8 [M,K] e4m3 (row scale sa), B4 [N or 2N, K/2] packed
// e2m1 (row stride ldb bytes), SB [N or 2N, K/32] E8M0 bytes (row stride lds bytes).
// Decode W4A16 (M <= 64, x_bf16 != null): C = epi(x . dequant(B4, SB)^T); A8/sa ignored.
// N = output columns; for EPI_SILU_MUL the weight has 2N rows in the packed [64 gate | 64 up] tile layout.
RAGK_API int ragk_gemm_mxfp4(const void* x_bf16, int ldx, const void* A8, int lda, const float* sa, const void* B4,
                             int ldb, const void* SB, int lds, void* C, int ldc, const void* bias, const void* resid,
                             int ldr, int M, int N, int K, int epi, int out_f32, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (K % 128 || ldb % 16 || ldb < K / 2 || lds % 4 || lds < K / 32 || (size_t)SB % 4) return (int)hipErrorInvalidValue;
  const bool dec = x_bf16 != nullptr;
  if (dec && M > 64) return (int)hipErrorInvalidValue;
  if (epi == EPI_SILU_MUL) {
    if (N % 64 || out_f32) return (int)hipErrorInvalidValue;
    return dec ? (int)dispatch_dec4<EPI_SILU_MUL, false>(x_bf16, ldx, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M,
                                                         N, K, st)
               : (int)launch_tile4<EPI_SILU_MUL, false>(A8, lda, sa, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M,
                                                        2 * N, K, st);
  }
  if (!dec && N % 8) return (int)hipErrorInvalidValue;
#define RAGK_MXFP4_CASE(E)                                                                                        \
  case E:                                                                                                         \
    if (dec)                                                                                                      \
      return out_f32                                                                                              \
                 ? (int)dispatch_dec4<E, true>(x_bf16, ldx, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M, N, K, st) \
                 : (int)dispatch_dec4<E, false>(x_bf16, ldx, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M, N, K, st); \
    return out_f32 ? (int)launch_tile4<E, true>(A8, lda, sa, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M, N, K, st) \
                   : (int)launch_tile4<E, false>(A8, lda, sa, B4, ldb, SB, lds, C, ldc, bias, resid, ldr, M, N, K, st);
  switch (epi) {
    RAGK_MXFP4_CASE(EPI_NONE)
    RAGK_MXFP4_CASE(EPI_BIAS)
    RAGK_MXFP4_CASE(EPI_RESID)
    RAGK_MXFP4_CASE(EPI_BIAS_RESID)
    RAGK_MXFP4_CASE(EPI_BIAS_GELU)
    RAGK_MXFP4_CASE(EPI_GELU)
    RAGK_MXFP4_CASE(EPI_BIAS_GELU_TANH)
    default: return (int)hipErrorInvalidValue;
  }
#undef RAGK_MXFP4_CASE
}
