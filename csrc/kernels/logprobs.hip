// Per-token log-probabilities with top-N alternatives for gfx950 (opt-in per request).
//
// logprob(t) = x[t] - lse(x) over the fp32 logits row x the sampler receives (after the logit processors,
// before temperature / top-k / top-p): log_softmax of the unwarped model distribution. Two launches:
//   1. lse_partials: workgroup (chunk c, row b) reduces its vocab chunk to (m, s) = (max, sum exp(x - m));
//      runs next to topk_candidates, on the same logits view (a vocab shard under tensor parallelism);
//   2. logprobs_finish: one workgroup per row folds the (all-gathered, rank-major) partials into lse, looks the
//      sampled token up in the candidate lists the sampler got, and merges the first N entries of every
//      sorted list into the global top N (value descending, vocabulary id ascending).
// Deterministic: no atomics, every reduction in a fixed order (a thread's elements in address order, lanes
// by the xor tree, waves / partials in ascending index), so the bits do not depend on the dispatch order.
// -inf logits are legal (the processors write them); NaN and +inf are not inputs.
#include "common.h"
#include <math.h>
using namespace ragk;

namespace {

constexpr int LSE_THREADS = 512;
constexpr int LSE_WAVES = LSE_THREADS / 64;
constexpr int LP_MAX = 20;        // alternatives per position (LOGPROBS_MAX)
constexpr int LP_MAX_PARTS = 512;  // partials per row: 64 chunks x 8 tensor-parallel ranks

// Chunk c of row b: [c0, c0 + n) with the top-k's chunk width (a multiple of 8). The chunk is read as
// a scalar head up to the first 16-byte boundary, 16-byte vectors, and a scalar tail (V = 1001 rows and
// strided views start anywhere); twice -- an exact block maximum first, then the sum of expf(x - m) --
// the second pass out of L2 (a chunk is 16-72 KB at the engine's chunking). The chunk is not held in registers
// between the passes: `chunks` is any of 1..64, so a thread's share has no fixed size (250 floats at V = 128256,
// one chunk), and the launch takes 3.5 us at batch 1, 5.7 us at batch 32 as it is (docs/PERF_NOTES.md "Logprobs").
__global__ __launch_bounds__(LSE_THREADS) void lse_partials_kernel(const float* __restrict__ logits, int ld, int Vtot,
                                                                   int chunks, float* __restrict__ part) {
  __shared__ float red_m[LSE_WAVES], red_s[LSE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int Vc = ((Vtot + chunks - 1) / chunks + 7) & ~7;
  const int c0 = min(chunk * Vc, Vtot);
  const int n = min(Vtot - c0, Vc);
  float* out = part + ((size_t)b * chunks + chunk) * 2;
  if (n <= 0) {  // block-uniform: an empty chunk of a short row
    if (tid == 0) { out[0] = -INFINITY; out[1] = 0.f; }
    return;
  }
  const float* row = logits + (size_t)b * ld + c0;
  const int head = min(n, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u));
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec, ntail = n - tail0;  // head, ntail in 0..3
  const f32x4* vrow = reinterpret_cast<const f32x4*>(row + head);

  float m = -INFINITY;
  for (int i = tid; i < nvec; i += LSE_THREADS) {
    const f32x4 v = vrow[i];
    m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  if (tid < head) m = fmaxf(m, row[tid]);
  if (tid < ntail) m = fmaxf(m, row[tail0 + tid]);
  m = wave_max(m);
  if (lane == 0) red_m[wid] = m;
  __syncthreads();
  m = red_m[0];
#pragma unroll
  for (int w = 1; w < LSE_WAVES; ++w) m = fmaxf(m, red_m[w]);
  if (m == -INFINITY) {  // block-uniform: every entry -inf (x - m would be inf - inf)
    if (tid == 0) { out[0] = -INFINITY; out[1] = 0.f; }
    return;
  }

  float s = 0.f;
  for (int i = tid; i < nvec; i += LSE_THREADS) {
    const f32x4 v = vrow[i];
    s += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
  }
  if (tid < head) s += expf(row[tid] - m);
  if (tid < ntail) s += expf(row[tail0 + tid] - m);
  s = wave_sum(s);
  if (lane == 0) red_s[wid] = s;
  __syncthreads();
  if (tid == 0) {
    float t = red_s[0];
#pragma unroll
    for (int w = 1; w < LSE_WAVES; ++w) t += red_s[w];
    out[0] = m;
    out[1] = t;
  }
}

// One workgroup of four waves per row b (nlp[b] < 0: nothing of the row is written).
//   top N: lists are sorted (value desc, id asc), so only the first N entries of each can be among the global
//   first N; lane l < N holds entry l of a list as the key (-value, id). Wave w folds lists w, w + 4, ... into
//   its running sorted list by the lane merge network the sampler uses (ties -> lower id; the next list's
//   entries are requested before the current one is merged), then wave 0 folds the four. The merged list is a
//   function of the candidate set alone (a total order), so the split over waves cannot change a bit.
//   By wave 0:
//   lse: M = max_p m_p; S = sum over ascending p of s_p * expf(m_p - M) (m_p = -inf adds 0); M + logf(S).
//   token: the one candidate whose id is tok[b] -> v - lse (NaN if it is in no list: loud).
// One wave for all of it took 18.4 us alone at 31 lists (31 dependent load + merge rounds; a development run of
// tools/logprobs_probe.py whose output was not kept); this form 10.6 us (profiles/logprobs_probe.log, batch 1,
// V = 128256).
constexpr int LF_WAVES = 4;

__global__ __launch_bounds__(64 * LF_WAVES) void logprobs_finish_kernel(
    const float* __restrict__ part, int P, const float* __restrict__ cand_v, const int* __restrict__ cand_i,
    int n_cand, int list_len, const int* __restrict__ tok, const int* __restrict__ nlp, float* __restrict__ out_lse,
    float* __restrict__ out_tok_lp, float* __restrict__ out_top_lp, int* __restrict__ out_top_id) {
  __shared__ float term[LP_MAX_PARTS];
  __shared__ float mv[LF_WAVES][64];
  __shared__ int mi[LF_WAVES][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int N = min(nlp[b], LP_MAX);
  if (N < 0) return;  // block-uniform
  const float* cv = cand_v + (size_t)b * n_cand;
  const int* ci = cand_i + (size_t)b * n_cand;

  float bv = INFINITY;  // running list, ascending by (-value, id); padding (+inf, -1) sorts last
  int bi = -1;
  if (N > 0) {  // block-uniform
    const int R = n_cand / list_len;
    const bool ok = lane < N;  // N <= list_len (checked by the launcher)
    int nid = (ok && w < R) ? ci[w * list_len + lane] : -1;
    float nv = (ok && w < R) ? cv[w * list_len + lane] : -INFINITY;
    for (int r = w; r < R; r += LF_WAVES) {
      const int id = nid;
      const float v = nv;
      const int rn = r + LF_WAVES;
      nid = (ok && rn < R) ? ci[rn * list_len + lane] : -1;
      nv = (ok && rn < R) ? cv[rn * list_len + lane] : -INFINITY;
      wave_merge64(bv, bi, id >= 0 ? -v : INFINITY, id, lane);
    }
    mv[w][lane] = bv;
    mi[w][lane] = bi;
    __syncthreads();
  }
  if (w != 0) return;
  if (N > 0) {
#pragma unroll
    for (int g = 1; g < LF_WAVES; ++g) wave_merge64(bv, bi, mv[g][lane], mi[g][lane], lane);
  }

  const float* pr = part + (size_t)b * P * 2;
  float M = -INFINITY;
  for (int p = lane; p < P; p += 64) M = fmaxf(M, pr[2 * p]);
  M = wave_max(M);
  for (int p = lane; p < P; p += 64) {
    const float mp = pr[2 * p], sp = pr[2 * p + 1];
    term[p] = mp == -INFINITY ? 0.f : sp * expf(mp - M);
  }
  // only wave 0 is left: its LDS operations complete in order, so the reads below see term[] once the compiler
  // keeps them behind the writes
  __builtin_amdgcn_wave_barrier();
  float S = 0.f;
  for (int p = 0; p < P; ++p) S += term[p];  // ascending p, the same chain in every lane
  const float lse = M + logf(S);

  const int t = tok[b];
  int hit = n_cand;  // lowest candidate index holding the token
  for (int j = lane; j < n_cand; j += 64)
    if (ci[j] == t) hit = min(hit, j);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hit = min(hit, __shfl_xor(hit, o, 64));
  if (lane == 0) {
    out_lse[b] = lse;
    out_tok_lp[b] = (t >= 0 && hit < n_cand) ? cv[hit] - lse : __int_as_float(0x7fc00000);
  }
  if (lane < N) {
    const float v = bi >= 0 ? -bv : -INFINITY;
    out_top_id[(size_t)b * LP_MAX + lane] = bi;
    out_top_lp[(size_t)b * LP_MAX + lane] = v - lse;
  }
}

}  // namespace

RAGK_API int ragk_logprobs_max() { return LP_MAX; }

// part: [B][chunks][2] fp32 (m, s). logits: fp32 rows of V entries, pitch ld (any alignment).
RAGK_API int ragk_lse_partials(const float* logits, int ld, int B, int V, int chunks, float* part, hipStream_t st) {
  if (B <= 0) return 0;
  if (V < 1 || chunks < 1 || chunks > 64 || B > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lse_partials_kernel, dim3(chunks, B), dim3(LSE_THREADS), 0, st, logits, ld, V, chunks, part);
  return (int)hipGetLastError();
}

// part: [B][P][2]; cand_v / cand_i: [B][n_cand] as n_cand / list_len sorted lists; out_top_*: [B][LP_MAX].
RAGK_API int ragk_logprobs_finish(const float* part, int P, const float* cand_v, const int* cand_i, int B, int n_cand,
                                  int list_len, const int* tok, const int* nlp, float* out_lse, float* out_tok_lp,
                                  float* out_top_lp, int* out_top_id, hipStream_t st) {
  if (B <= 0) return 0;
  if (P < 1 || P > LP_MAX_PARTS || n_cand < 1 || list_len < LP_MAX || n_cand % list_len)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(logprobs_finish_kernel, dim3(B), dim3(64 * LF_WAVES), 0, st, part, P, cand_v, cand_i, n_cand, list_len, tok,
                     nlp, out_lse, out_tok_lp, out_top_lp, out_top_id);
  return (int)hipGetLastError();
}
