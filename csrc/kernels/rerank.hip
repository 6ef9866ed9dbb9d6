// Cross-encoder reranking kernels for gfx950: BERT embeddings with per-token type ids, the
// sequence-classification head as one launch, and a segmented stable top-k by score.
//
//   embed_ln_tt    LN(word[id] + pos[pos_id] + type_table[type_id]); the arithmetic (and its order) is
//                  that of embed_ln_kernel in norm.hip, so all-zero type ids reproduce it bit for bit.
//   cls_head       score[b] = w2 . tanh(W1 . h[cu[b]] + b1) + b2 for a tile of 16 sequences per
//                  workgroup: the 16 CLS rows are gathered once into LDS as the MFMA A operand, the four
//                  waves sweep the H output columns (16 per 16x16x32 bf16 MFMA tile, K = H), bias + tanh
//                  + the w2 product stay in registers, and lanes then waves are reduced in a fixed order.
//                  W1 is read once per 16 sequences instead of once per sequence.
//   rerank_select  one wave per query, one lane per candidate: a lane's output slot is the number of
//                  candidates that beat it (higher score, or equal score and earlier position), which is
//                  a stable descending sort without any exchange network.
#include <float.h>

#include "common.h"
using namespace ragk;

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void embed_ln_tt_kernel(const int* __restrict__ ids, const int* __restrict__ pos_ids,
                                                         const int* __restrict__ type_ids,
                                                         const bf16_t* __restrict__ word,
                                                         const bf16_t* __restrict__ pos,
                                                         const bf16_t* __restrict__ type_table, int type_vocab,
                                                         const bf16_t* __restrict__ g, const bf16_t* __restrict__ b,
                                                         bf16_t* out, int H, float eps) {
  __shared__ float red[NT / 64];
  const int t = blockIdx.x;
  const bf16_t* wr = word + (size_t)ids[t] * H;
  const bf16_t* pr = pos + (size_t)pos_ids[t] * H;
  const int ty_id = min(max(type_ids[t], 0), type_vocab - 1);
  const bf16_t* type = type_table + (size_t)ty_id * H;
  constexpr int MAXV = 4;
  float v[MAXV][8];
  const int nvec = H >> 3;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) {
      float a[8], p[8], ty[8];
      unpack8(*reinterpret_cast<const u32x4*>(wr + vi * 8), a);
      unpack8(*reinterpret_cast<const u32x4*>(pr + vi * 8), p);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = a[e] + p[e];
      unpack8(*reinterpret_cast<const u32x4*>(type + vi * 8), ty);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] += ty[e];
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    }
  }
  const float mean = block_sum(s, red) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[i][e] - mean;
        sq += d * d;
      }
  }
  const float inv = rsqrtf(block_sum(sq, red) / (float)H + eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) {
      float gv[8], bv[8], o[8];
      unpack8(*reinterpret_cast<const u32x4*>(g + vi * 8), gv);
      unpack8(*reinterpret_cast<const u32x4*>(b + vi * 8), bv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * inv * gv[e] + bv[e];
      *reinterpret_cast<u32x4*>(out + (size_t)t * H + vi * 8) = pack8(o);
    }
  }
}

// ---- classification head ----------------------------------------------------------------------------
constexpr int CH_ROWS = 16;     // sequences per workgroup = one MFMA m-tile
constexpr int CH_MAXH = 1024;
constexpr int CH_PAD = 8;       // bf16 elements of row padding: 16 rows at one k land in distinct banks

__global__ __launch_bounds__(NT) void cls_head_kernel(const bf16_t* __restrict__ h, int ld, int T,
                                                      const int* __restrict__ cu, const bf16_t* __restrict__ W1,
                                                      const bf16_t* __restrict__ b1, const bf16_t* __restrict__ w2,
                                                      float b2, float* __restrict__ out, int B, int H) {
  __shared__ __attribute__((aligned(16))) bf16_t xs[CH_ROWS * (CH_MAXH + CH_PAD)];
  __shared__ float part[NT / 64][CH_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int b0 = blockIdx.x * CH_ROWS;
  const int pitch = H + CH_PAD;
  const int nvec = H >> 3;

  // gather the tile's CLS rows (rows past B repeat the last sequence's; their scores are not written)
  for (int i = tid; i < CH_ROWS * nvec; i += NT) {
    const int r = i / nvec, vi = i - r * nvec;
    const int row = min(max(cu[min(b0 + r, B - 1)], 0), T - 1);
    *reinterpret_cast<u32x4*>(xs + r * pitch + vi * 8) =
        *reinterpret_cast<const u32x4*>(h + (size_t)row * ld + vi * 8);
  }
  __syncthreads();

  float sum[4] = {0.f, 0.f, 0.f, 0.f};  // rows 4*fh + r, this lane's columns
  const int ntiles = H >> 4;
  for (int nt = wid; nt < ntiles; nt += NT / 64) {
    const int col = nt * 16 + fr;
    const bf16_t* wp = W1 + (size_t)col * H + fh * 8;
    const bf16_t* xp = xs + fr * pitch + fh * 8;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < H; k += 32) {
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xp + k);
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wp + k);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, wf, acc, 0, 0, 0);
    }
    const float bias = bf2f(b1[col]), wo = bf2f(w2[col]);
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] += wo * tanhf(acc[r] + bias);
  }
  // the 16 lanes that share fh hold the same rows: butterfly over fr, then the waves in order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum[r] += __shfl_xor(sum[r], o, 64);
  }
  if (fr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wid][4 * fh + r] = sum[r];
  }
  __syncthreads();
  if (tid < CH_ROWS && b0 + tid < B) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += part[w][tid];
    out[b0 + tid] = s + b2;
  }
}

// ---- segmented stable top-k by score -----------------------------------------------------------------
constexpr int SEL_WAVES = 4;  // queries per workgroup

// j (earlier or later position pj) ranks ahead of i: finite/inf scores descending, NaN last, ties by position
__device__ __forceinline__ bool beats(float sj, int pj, float si, int pi) {
  const bool nj = sj != sj, ni = si != si;
  const bool first = pj < pi;
  if (nj) return ni & first;
  if (ni) return true;
  return (sj > si) | ((sj == si) & first);
}

__global__ __launch_bounds__(64 * SEL_WAVES) void rerank_select_kernel(
    const float* __restrict__ scores, const long long* __restrict__ cand_ids, const float* __restrict__ cand_dist,
    const int* __restrict__ n_valid, long long* __restrict__ out_ids, float* __restrict__ out_dist,
    float* __restrict__ out_score, int Q, int N, int k) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
  if (q >= Q) return;  // wave-uniform
  const int nv = min(max(n_valid[q], 0), N);
  const bool valid = lane < nv;
  const size_t base = (size_t)q * N;
  const float s = valid ? scores[base + lane] : 0.f;
  int rank = 0;
  for (int j = 0; j < nv; ++j) {  // nv is wave-uniform
    const float sj = __shfl(s, j, 64);
    rank += (j != lane && beats(sj, j, s, lane)) ? 1 : 0;
  }
  const size_t ob = (size_t)q * k;
  if (valid && rank < k) {
    out_ids[ob + rank] = cand_ids[base + lane];
    out_dist[ob + rank] = cand_dist[base + lane];
    out_score[ob + rank] = s;
  }
  if (lane >= nv && lane < k) {
    out_ids[ob + lane] = -1;
    out_dist[ob + lane] = FLT_MAX;
    out_score[ob + lane] = -FLT_MAX;
  }
}

}  // namespace

RAGK_API int ragk_embed_ln_tt(const int* ids, const int* pos_ids, const int* type_ids, const void* word,
                              const void* pos, const void* type_table, int type_vocab, const void* g, const void* b,
                              void* out, int T, int H, float eps, hipStream_t st) {
  if (T <= 0) return 0;
  if (H % 8 || H > 8 * NT * 4 || type_vocab < 1 || !type_ids || !type_table || !g || !b)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_ln_tt_kernel, dim3(T), dim3(NT), 0, st, ids, pos_ids, type_ids, (const bf16_t*)word,
                     (const bf16_t*)pos, (const bf16_t*)type_table, type_vocab, (const bf16_t*)g, (const bf16_t*)b,
                     (bf16_t*)out, H, eps);
  return (int)hipGetLastError();
}

// h: [T, ld] bf16 packed hidden states, cu: int32 [B + 1], W1: [H, H] bf16 row-major (out, in), b1 / w2: [H] bf16.
RAGK_API int ragk_cls_head(const void* h, int ld, int T, const int* cu, const void* W1, const void* b1,
                           const void* w2, float b2, float* out, int B, int H, hipStream_t st) {
  if (B <= 0) return 0;
  if (H % 64 || H < 64 || H > CH_MAXH || T < 1 || ld < H || ld % 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cls_head_kernel, dim3((B + CH_ROWS - 1) / CH_ROWS), dim3(NT), 0, st, (const bf16_t*)h, ld, T, cu,
                     (const bf16_t*)W1, (const bf16_t*)b1, (const bf16_t*)w2, b2, out, B, H);
  return (int)hipGetLastError();
}

RAGK_API int ragk_rerank_select(const float* scores, const long long* cand_ids, const float* cand_dist,
                                const int* n_valid, long long* out_ids, float* out_dist, float* out_score, int Q,
                                int N, int k, hipStream_t st) {
  if (Q <= 0) return 0;
  if (N < 1 || N > 64 || k < 1 || k > N) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rerank_select_kernel, dim3((Q + SEL_WAVES - 1) / SEL_WAVES), dim3(64 * SEL_WAVES), 0, st, scores,
                     cand_ids, cand_dist, n_valid, out_ids, out_dist, out_score, Q, N, k);
  return (int)hipGetLastError();
}
