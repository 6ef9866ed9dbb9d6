// History-dependent logit processors for gfx950, applied in place on the fp32 logits between lm_head and
// the candidate top-k, inside the decode graph: transformers' RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor, in that order.
//
// The token history is a device buffer hist[rows][ld] (int32) whose every write is
// hist[row][position] = token at that position: writes are idempotent, so a decode step that is discarded and
// recomputed rewrites the same cells with the right ids, and a stale cell past a row's length is never read.
// Nothing accumulates (no counts, no bitmaps).
#include "common.h"
#include <math.h>
using namespace ragk;

namespace {

// 1024 threads per row: the passes are chains of dependent loads (history id -> its logit), ~5 entries per
// thread at a 5.2k-token history. Alone in a graph at batch 1 / 32, V = 128256: 9.8 / 11.1 us; with 256
// threads (~20 entries per thread) 20.9 / 22.4 us (profiles/logits_proc_probe.log).
constexpr int LP_THREADS = 1024;
constexpr int LP_MAX_HIST = 32768;  // history entries staged in LDS per row (128 KiB of the 160 KiB)
constexpr int LP_MAX_NGRAM = 8;

// prefill scatter: hist[rows[i]][pos[i]] = ids[i]; rows < 0 (sequences without processors) are skipped
__global__ __launch_bounds__(LP_THREADS) void hist_write_kernel(const int* __restrict__ ids, const int* __restrict__ rows,
                                                                const int* __restrict__ pos, int* __restrict__ hist,
                                                                int hist_rows, int ld, int T) {
  const int i = blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= T) return;
  const int r = rows[i], p = pos[i];
  if (r < 0 || r >= hist_rows || p < 0 || p >= ld) return;
  hist[(size_t)r * ld + p] = ids[i];
}

// One workgroup (LP_THREADS threads) per logits row b (history row rows[b], length pos[b] + 1).
//   1. rows[b] < 0: nothing is touched (padded graph rows, rows of requests without processors).
//   2. ids given (decode): hist[row][pos[b]] = ids[b] first -- ids[b] is the id the embedding kernel
//      resolved (carried rows included), so this launch comes after the embedding.
//   3. repetition penalty: every history entry's ORIGINAL logit is staged in LDS before any thread of the row
//      writes one; then every entry writes f(original). Duplicate ids write the same value, so the
//      penalty applies once per distinct id without atomics or a dedupe pass.
//   4. after a barrier: the -inf writes of the n-gram ban and of the min_new_tokens ban list.
// Ids outside [vocab_offset, vocab_offset + V) belong to another tensor-parallel vocab shard and are skipped.
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(
    float* logits, int ld, int V, int vocab_offset, const int* __restrict__ ids,
    const int* __restrict__ rows, const int* __restrict__ pos, int* hist, int hist_rows, int hist_ld,
    const float* __restrict__ penalty, const int* __restrict__ ngram, const int* __restrict__ ban_ids, int ban_ld,
    const int* __restrict__ ban_count) {
  extern __shared__ float stage[];  // hist_ld floats
  const int b = blockIdx.x, tid = threadIdx.x;
  const int row = rows[b];
  if (row < 0 || row >= hist_rows) return;  // block-uniform
  const int p = pos[b];
  int* h = hist + (size_t)row * hist_ld;
  if (ids != nullptr) {
    if (tid == 0 && p >= 0 && p < hist_ld) h[p] = ids[b];
    __syncthreads();  // the store above is visible to the whole workgroup below
  }
  const int L = min(max(p + 1, 0), hist_ld);
  float* lrow = logits + (size_t)b * ld;

  const float pen = penalty[b];
  if (pen != 1.0f) {  // block-uniform; x * 1 and x / 1 are x, so skipping is exact
#pragma unroll 4
    for (int i = tid; i < L; i += LP_THREADS) {
      const int t = h[i] - vocab_offset;
      stage[i] = (t >= 0 && t < V) ? lrow[t] : 0.f;
    }
    __syncthreads();  // every original logit is read before any is written
#pragma unroll 4
    for (int i = tid; i < L; i += LP_THREADS) {
      const int t = h[i] - vocab_offset;
      if (t >= 0 && t < V) {
        const float x = stage[i];
        lrow[t] = x < 0.f ? x * pen : x / pen;
      }
    }
    __syncthreads();  // the -inf writes below win over the penalty
  }

  const int n = ngram[b];
  if (n >= 1 && n <= LP_MAX_NGRAM && L >= n) {
    // the last n-1 tokens; every earlier occurrence of them bans the token that followed it
    const int* suf = h + (L - n + 1);
    for (int j = tid; j <= L - n; j += LP_THREADS) {
      bool match = true;
      for (int k = 0; k < n - 1; ++k) match &= h[j + k] == suf[k];
      if (match) {
        const int t = h[j + n - 1] - vocab_offset;
        if (t >= 0 && t < V) lrow[t] = -INFINITY;
      }
    }
  }
  const int nb = min(ban_count[b], ban_ld);
  for (int i = tid; i < nb; i += LP_THREADS) {
    const int t = ban_ids[(size_t)b * ban_ld + i] - vocab_offset;
    if (t >= 0 && t < V) lrow[t] = -INFINITY;
  }
}

}  // namespace

RAGK_API int ragk_logits_proc_max_hist() { return LP_MAX_HIST; }

RAGK_API int ragk_hist_write(const int* ids, const int* rows, const int* pos, int* hist, int hist_rows, int ld, int T,
                             hipStream_t st) {
  if (T <= 0) return 0;
  if (hist_rows < 1 || ld < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hist_write_kernel, dim3((T + LP_THREADS - 1) / LP_THREADS), dim3(LP_THREADS), 0, st, ids, rows,
                     pos, hist, hist_rows, ld, T);
  return (int)hipGetLastError();
}

// ids may be null (prefill's sampled rows: the history is already complete, length pos[b] + 1).
// ban_ids: [B][ban_ld]; ban_count[b] = 0 once row b has generated min_new_tokens.
RAGK_API int ragk_logits_process(float* logits, int ld, int B, int V, int vocab_offset, const int* ids,
                                 const int* rows, const int* pos, int* hist, int hist_rows, int hist_ld,
                                 const float* penalty, const int* ngram, const int* ban_ids, int ban_ld,
                                 const int* ban_count, hipStream_t st) {
  if (B <= 0) return 0;
  if (V < 1 || ld < V || hist_rows < 1 || hist_ld < 1 || hist_ld > LP_MAX_HIST || ban_ld < 1)
    return (int)hipErrorInvalidValue;
  static bool attr = false;  // > 64 KiB of dynamic LDS needs the opt-in
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)logits_process_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, LP_MAX_HIST * 4);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(logits_process_kernel, dim3(B), dim3(LP_THREADS), (size_t)hist_ld * 4, st, logits, ld, V,
                     vocab_offset, ids, rows, pos, hist, hist_rows, hist_ld, penalty, ngram, ban_ids, ban_ld,
                     ban_count);
  return (int)hipGetLastError();
}
