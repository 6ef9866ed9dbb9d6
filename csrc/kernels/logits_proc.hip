// History-dependent logit processors for gfx950, applied in place on the fp32 logits between lm_head and
// the candidate top-k, inside the decode graph: transformers' RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor, in that order.
//
// The token history is a device buffer hist[rows][ld] (int32) whose every write is
// hist[row][position] = token at that position: writes are idempotent, so a decode step that is discarded and
// recomputed rewrites the same cells with the right ids, and a stale cell past a row's length is never read.
// Nothing accumulates (no counts, no bitmaps) in global memory: the counts of the frequency / presence penalties
// live in LDS for the length of one launch.
//
// One chain, two entry points. Per logits row: history store, [logit_bias], repetition penalty, [frequency /
// presence over the GENERATED tokens], then the -inf writes of the n-gram ban and the ban list. The bracketed
// phases are the OpenAI-style controls; only logits_process_pen_kernel has them, so a step without such a row
// launches logits_process_kernel and pays nothing for them. The phases both kernels run are the lp_* device
// functions below, which take plain values and pointers (each kernel keeps its own early exit and history
// store: the kernarg loads then stay where they are needed).
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
constexpr int LP_PEN_GEN_MAX = 8192;                  // generated tokens a penalty row may count
constexpr int LP_PEN_MAX_SLOTS = 2 * LP_PEN_GEN_MAX;  // counting table: load <= 1/2, 8 B per slot = 128 KiB
constexpr int LP_PEN_MIN_SLOTS = 64;
constexpr int LP_BIAS_MAX = 300;

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

// Repetition penalty of one row (history h[0 .. L), logits lrow): every history entry's ORIGINAL logit is staged
// in LDS before any thread of the row writes one; then every entry writes f(original). Duplicate ids write the
// same value, so the penalty applies once per distinct id without atomics or a dedupe pass. Ends in a barrier:
// later writes win over the penalty, and the stage is free.
__device__ __forceinline__ void lp_repetition(float* lrow, int V, int vocab_offset, const int* h, int L, float pen,
                                              float* stage, int tid) {
  if (pen == 1.0f) return;  // block-uniform; x * 1 and x / 1 are x, so skipping is exact
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
  __syncthreads();
}

// The -inf writes of one row: the n-gram ban (size n) over its history, then the first min(*ban_count, ban_ld) ids
// of its ban list (min_new_tokens). The count is read here, after the n-gram pass, where the kernels always read it.
__device__ __forceinline__ void lp_bans(float* lrow, int V, int vocab_offset, const int* h, int L, int n,
                                        const int* __restrict__ ban, int ban_ld, const int* __restrict__ ban_count,
                                        int tid) {
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
  const int nb = min(*ban_count, ban_ld);
  for (int i = tid; i < nb; i += LP_THREADS) {
    const int t = ban[i] - vocab_offset;
    if (t >= 0 && t < V) lrow[t] = -INFINITY;
  }
}

// One workgroup (LP_THREADS threads) per logits row b (history row rows[b], length pos[b] + 1).
//   1. rows[b] < 0: nothing is touched (padded graph rows, rows of requests without processors).
//   2. ids given (decode): hist[row][pos[b]] = ids[b] first -- ids[b] is the id the embedding kernel
//      resolved (carried rows included), so this launch comes after the embedding.
//   3. repetition penalty (lp_repetition).
//   4. the -inf writes of the n-gram ban and of the min_new_tokens ban list (lp_bans).
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

  lp_repetition(lrow, V, vocab_offset, h, L, penalty[b], stage, tid);
  lp_bans(lrow, V, vocab_offset, h, L, ngram[b], ban_ids + (size_t)b * ban_ld, ban_ld, ban_count + b, tid);
}

// Counting table of the frequency / presence penalties: open addressing with linear probing over `slots` (a power
// of two) keys and counts in LDS, aliased onto the repetition phase's stage once that phase has passed its last
// barrier. A hash table and not a sort or a first-occurrence scan: one pass over the generated span, ~8 entries
// per thread at the 8192-token bound, and the work of a 150-token answer is a 512-slot clear plus one insert
// per lane of three waves. Integer atomics only, so the counts do not depend on arrival order; which slot an id
// lands in may, but every occupied slot writes its own id's logit exactly once.
__device__ __forceinline__ unsigned lp_hash(int t, int shift) { return ((unsigned)t * 2654435761u) >> shift; }

// (x - freq * c) - pres as three separately rounded fp32 operations. hipcc contracts a * b - c to an FMA by
// default, and __fmul_rn / __fsub_rn do not stop it (they are the plain operators here); the pragma does.
__device__ __forceinline__ float lp_freq_pres(float x, float freq, float c, float pres) {
#pragma clang fp contract(off)
  const float fc = freq * c;
  const float y = x - fc;
  return y - pres;
}

// The chain with its optional phases, logit_bias and the frequency / presence penalties:
//   1. early exit and history store (decode), as above.
//   2. bias: thread i < bias_count[b] adds bias_vals[row][i] to the logit of bias_ids[row][i]. The ids of a table
//      row are distinct (admission), so one read-add-write per thread needs no atomics. The tables are indexed
//      by the HISTORY row: they are written once per sequence, not per step.
//   3. repetition penalty (lp_repetition), on the biased values.
//   4. frequency, then presence, over the generated tokens h[gen_start .. L): every distinct id t with count c
//      gets (x - frequency * float(c)) - presence, three separately rounded fp32 operations (what torch's
//      x -= f * c; x -= p computes; no FMA contraction). Skipped block-uniformly when both are 0.
//   5. the -inf writes (lp_bans), which win.
// The table takes min(tslots, the power of two >= 2 * generated) slots; the launcher sizes tslots for the host's
// bound on the generated span. A row whose span exceeds its table (the host's bound was wrong) loses counts, it
// never loops: every probe run is bounded by the slot count.
__global__ __launch_bounds__(LP_THREADS) void logits_process_pen_kernel(
    float* logits, int ld, int V, int vocab_offset, const int* __restrict__ ids,
    const int* __restrict__ rows, const int* __restrict__ pos, int* hist, int hist_rows, int hist_ld,
    const float* __restrict__ penalty, const int* __restrict__ ngram, const int* __restrict__ ban_ids, int ban_ld,
    const int* __restrict__ ban_count, const int* __restrict__ gen_start, const float* __restrict__ presence,
    const float* __restrict__ frequency, const int* __restrict__ bias_count, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_vals, int bias_ld, int tslots) {
  extern __shared__ float stage[];  // max(hist_ld floats, tslots keys + tslots counts)
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

  const int nbias = min(max(bias_count[b], 0), bias_ld);
  if (nbias > 0) {  // block-uniform
    for (int i = tid; i < nbias; i += LP_THREADS) {
      const int t = bias_ids[(size_t)row * bias_ld + i] - vocab_offset;
      if (t >= 0 && t < V) lrow[t] = lrow[t] + bias_vals[(size_t)row * bias_ld + i];
    }
    __syncthreads();  // the phases below read the biased values
  }

  lp_repetition(lrow, V, vocab_offset, h, L, penalty[b], stage, tid);  // the stage is free from here on

  const float pres = presence[b], freq = frequency[b];
  const int g0 = min(max(gen_start[b], 0), L);
  if ((pres != 0.0f || freq != 0.0f) && L > g0) {  // block-uniform
    int slots = LP_PEN_MIN_SLOTS, shift = 32 - 6;
    while (slots < 2 * (L - g0) && slots < tslots) slots <<= 1, --shift;
    const int mask = slots - 1;
    int* keys = reinterpret_cast<int*>(stage);
    int* cnts = keys + slots;
    for (int s = tid; s < slots; s += LP_THREADS) {
      keys[s] = -1;
      cnts[s] = 0;
    }
    __syncthreads();
    for (int i = g0 + tid; i < L; i += LP_THREADS) {
      const int t = h[i] - vocab_offset;
      if (t < 0 || t >= V) continue;
      int s = (int)lp_hash(t, shift);
      for (int probe = 0; probe < slots; ++probe) {  // claim, match or move on; never wait
        const int prev = atomicCAS(&keys[s], -1, t);
        if (prev == -1 || prev == t) {
          atomicAdd(&cnts[s], 1);
          break;
        }
        s = (s + 1) & mask;
      }
    }
    __syncthreads();  // every count is final
    for (int s = tid; s < slots; s += LP_THREADS) {
      const int t = keys[s];
      if (t >= 0) lrow[t] = lp_freq_pres(lrow[t], freq, (float)cnts[s], pres);
    }
    __syncthreads();  // the -inf writes below win over the penalties
  }

  lp_bans(lrow, V, vocab_offset, h, L, ngram[b], ban_ids + (size_t)b * ban_ld, ban_ld, ban_count + b, tid);
}

// What both launchers check of their arguments, and the opt-in to more than 64 KiB of dynamic LDS, taken once
// per kernel (*opted). 0, or the hipError_t to return.
int lp_prepare(const void* kernel, bool* opted, int ld, int V, int hist_rows, int hist_ld, int ban_ld) {
  if (V < 1 || ld < V || hist_rows < 1 || hist_ld < 1 || hist_ld > LP_MAX_HIST || ban_ld < 1)
    return (int)hipErrorInvalidValue;
  if (!*opted) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LP_MAX_HIST * 4);
    if (e != hipSuccess) return (int)e;
    *opted = true;
  }
  return 0;
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
  static bool attr = false;
  if (const int e = lp_prepare((const void*)logits_process_kernel, &attr, ld, V, hist_rows, hist_ld, ban_ld)) return e;
  hipLaunchKernelGGL(logits_process_kernel, dim3(B), dim3(LP_THREADS), (size_t)hist_ld * 4, st, logits, ld, V,
                     vocab_offset, ids, rows, pos, hist, hist_rows, hist_ld, penalty, ngram, ban_ids, ban_ld,
                     ban_count);
  return (int)hipGetLastError();
}

RAGK_API int ragk_logits_proc_pen_gen_max() { return LP_PEN_GEN_MAX; }
RAGK_API int ragk_logits_proc_bias_max() { return LP_BIAS_MAX; }

// ragk_logits_process with logit_bias and frequency / presence penalties (logits_process_pen_kernel). Its further
// per-row arguments: gen_start (prompt length), presence, frequency, bias_count [B]; bias_ids / bias_vals
// [hist_rows][bias_ld], indexed by history row. gen_bound: the host's bound on pos[b] - gen_start[b] + 1 over
// the rows with a penalty; it sizes the counting table and is refused above LP_PEN_GEN_MAX.
RAGK_API int ragk_logits_process_pen(float* logits, int ld, int B, int V, int vocab_offset, const int* ids,
                                     const int* rows, const int* pos, int* hist, int hist_rows, int hist_ld,
                                     const float* penalty, const int* ngram, const int* ban_ids, int ban_ld,
                                     const int* ban_count, const int* gen_start, const float* presence,
                                     const float* frequency, const int* bias_count, const int* bias_ids,
                                     const float* bias_vals, int bias_ld, int gen_bound, hipStream_t st) {
  if (B <= 0) return 0;
  if (bias_ld < 1 || gen_bound < 0 || gen_bound > LP_PEN_GEN_MAX) return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (const int e = lp_prepare((const void*)logits_process_pen_kernel, &attr, ld, V, hist_rows, hist_ld, ban_ld))
    return e;
  int tslots = LP_PEN_MIN_SLOTS;
  while (tslots < 2 * gen_bound) tslots <<= 1;  // <= LP_PEN_MAX_SLOTS
  const size_t lds = max((size_t)hist_ld * 4, (size_t)tslots * 8);
  hipLaunchKernelGGL(logits_process_pen_kernel, dim3(B), dim3(LP_THREADS), lds, st, logits, ld, V, vocab_offset, ids,
                     rows, pos, hist, hist_rows, hist_ld, penalty, ngram, ban_ids, ban_ld, ban_count, gen_start,
                     presence, frequency, bias_count, bias_ids, bias_vals, bias_ld, tslots);
  return (int)hipGetLastError();
}
