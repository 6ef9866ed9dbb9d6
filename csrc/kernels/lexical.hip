// BM25 lexical search for gfx950 over a doc-major CSR of (term id, tf) entries (index/lexical.py):
//   lex_df      live documents that contain each of <= 4096 sorted distinct query terms (integer counts)
//   lex_search  per query the top k documents by BM25 score (descending, ties -> lower id, padding id -1)
//
// The arithmetic is fixed so that ops/reference.py matches it bit for bit: every operation is rounded on its
// own (fp contract off, IEEE division), a document's score is the sum of its matching terms' contributions in
// ascending term-id order (= the order of its CSR entries), and nothing is accumulated with float atomics:
//   norm  = k1 * ((1 - b) + b * (float(dl) / avgdl))
//   c     = idf[t] * ((float(tf) * k1p1) / (float(tf) + norm))
//   score = c_0 + c_1 + ...
// idf and avgdl come from the host (float64 numpy from the lex_df counts), so both backends use the same numbers.
//
// lex_scan: a persistent grid, workgroups over tiles of 64 documents. The term table, idf and the 64-bit
// membership words (bit q = query q holds the term) are staged in LDS once per workgroup. Phase 1: one wave per
// document; its lanes stream the document's entries coalesced and binary-search the LDS table, a ballot
// names the hits in entry order, and LANE q adds the hits of QUERY q in that order (the contribution of a hit
// is wave-uniform; only the membership bit differs per lane). The scores go into an LDS tile [doc][query].
// Phase 2: the tile is read back one lane per document and offered, 64 candidates at a time, to per-query
// running top lists held one entry per lane (common.h wave_offer; skipped when no lane beats the k-th place);
// the 64 queries are split over the 4 waves, 16 lists per wave, in registers. Scores travel negated, so the
// lists' ascending order and (FLT_MAX, -1) padding apply. Each workgroup writes its lists as [nq][G][k] and
// lex_merge (one workgroup per query) reduces them.
#include "common.h"
#include <float.h>
using namespace ragk;

#pragma clang fp contract(off)

namespace {

constexpr int LT = 256;         // threads per workgroup (4 waves)
constexpr int LEX_TMAX = 4096;  // terms per launch (64 queries x 64 terms)
constexpr int TILE = 64;        // documents per tile
constexpr int TP = TILE + 1;    // pitch of the score tile in floats (transposed read: one bank per lane)
constexpr int DW = TILE / 4;    // documents per wave and tile
constexpr int QW = 16;          // query lists per wave (4 waves x 16 = 64 queries per launch)
constexpr int LMW = 16;         // waves of the merge workgroup

// position of `term` in the sorted table tt[0, T), or -1
__device__ __forceinline__ int lex_find(const unsigned* tt, int T, unsigned term) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tt[mid] < term) lo = mid + 1;
    else hi = mid;
  }
  return (lo < T && tt[lo] == term) ? lo : -1;
}

// Per-query id bitmaps, the format ragk_l2_search_masked takes: query j may only return ids whose bit is set in
// row qmask[j] of masks[n_masks][stride] (bit id & 31 of word id >> 5); qmask[j] < 0 (or qmask == nullptr) = no
// filter; an id outside [0, bits) is not allowed, so a short bitmap is never read out of bounds.
struct LexMask {
  const unsigned* masks;
  const int* qmask;
  int stride;
  int bits;
};

__device__ __forceinline__ unsigned lex_mask_word(const LexMask& m, int mr, bool ok, int id) {
  if (mr < 0) return ok ? ~0u : 0u;
  return (ok && (unsigned)id < (unsigned)m.bits) ? m.masks[(size_t)mr * m.stride + (id >> 5)] : 0u;
}

__device__ __forceinline__ float lex_contrib(float idf, float ftf, float k1p1, float norm) {
#pragma clang fp contract(off)
  const float num = ftf * k1p1;
  const float den = ftf + norm;
  const float r = num / den;
  return idf * r;
}

// df[t] += live documents holding qt[t]. One wave per document; hits are counted in LDS integers and every
// workgroup adds its non-zero counts to df with integer global atomics (df zeroed by the launcher).
__global__ __launch_bounds__(LT) void lex_df_kernel(const long long* __restrict__ row_ptr,
                                                    const unsigned* __restrict__ terms, int n,
                                                    const unsigned* __restrict__ qt, int T,
                                                    const unsigned* __restrict__ live, int live_bits,
                                                    int* __restrict__ df) {
  extern __shared__ __attribute__((aligned(16))) unsigned df_smem[];
  unsigned* tt = df_smem;                              // [T]
  int* cnt = reinterpret_cast<int*>(df_smem + T);      // [T]
  for (int i = threadIdx.x; i < T; i += LT) {
    tt[i] = qt[i];
    cnt[i] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long doc = (long long)blockIdx.x * 4 + w; doc < n; doc += (long long)gridDim.x * 4) {
    if (live) {  // wave-uniform
      const bool ok = doc < live_bits && ((live[doc >> 5] >> (doc & 31)) & 1u);
      if (!ok) continue;
    }
    const long long e0 = row_ptr[doc], e1 = row_ptr[doc + 1];
    for (long long e = e0 + lane; e < e1; e += 64) {
      const int t = lex_find(tt, T, terms[e]);
      if (t >= 0) atomicAdd(&cnt[t], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T; i += LT)
    if (cnt[i]) atomicAdd(&df[i], cnt[i]);
}

__global__ __launch_bounds__(LT) void lex_scan_kernel(const long long* __restrict__ row_ptr,
                                                      const unsigned* __restrict__ terms,
                                                      const unsigned short* __restrict__ tf,
                                                      const int* __restrict__ doc_len, int n, int ntiles,
                                                      const unsigned* __restrict__ qt, const float* __restrict__ idf,
                                                      const unsigned long long* __restrict__ member, int T, int nq,
                                                      float k1, float k1p1, float b, float avgdl, int k, LexMask mk,
                                                      float* __restrict__ out_v, int* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lx_smem[];
  unsigned long long* mem = reinterpret_cast<unsigned long long*>(lx_smem);  // [T]
  unsigned* tt = reinterpret_cast<unsigned*>(mem + T);                       // [T]
  float* idfs = reinterpret_cast<float*>(tt + T);                            // [T]
  float* tile = idfs + T;                                                    // [TILE][TP]
  for (int i = threadIdx.x; i < T; i += LT) {
    mem[i] = member[i];
    tt[i] = qt[i];
    idfs[i] = idf[i];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float bv[QW];
  int bi[QW], mr[QW];
#pragma unroll
  for (int j = 0; j < QW; ++j) {
    bv[j] = FLT_MAX;
    bi[j] = -1;
    const int q = w * QW + j;
    mr[j] = (mk.qmask && q < nq) ? mk.qmask[q] : -1;  // wave-uniform
  }
  const float omb = 1.0f - b;
  __syncthreads();
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int d0 = ti * TILE;
    // ---- phase 1: wave w scores documents d0 + DW * w .. + DW - 1; lane = query
    const int dw0 = d0 + DW * w;
    // the wave's row pointers and lengths in one load each (lane l: document dw0 + l), handed out by shuffles
    const long long rp = row_ptr[min(dw0 + lane, n)];  // lanes past DW read valid entries they never use
    const int dlv = doc_len[min(dw0 + lane, n - 1)];
    for (int dd = 0; dd < DW; ++dd) {
      const int doc = dw0 + dd;
      float acc = 0.f;
      bool any = false;
      const long long e0 = __shfl(rp, dd, 64), e1 = __shfl(rp, dd + 1, 64);
      const float dl = (float)__shfl(dlv, dd, 64);
      if (doc < n) {  // wave-uniform
        const float norm = k1 * (omb + b * (dl / avgdl));
        for (long long e = e0; e < e1; e += 64) {
          const long long le = e + lane;
          int t = -1;
          unsigned tfv = 0;
          if (le < e1) {
            t = lex_find(tt, T, terms[le]);
            tfv = tf[le];
          }
          unsigned long long hb = __ballot(t >= 0);
          const int packed = t >= 0 ? (int)(((unsigned)t << 16) | tfv) : 0;
          while (hb) {  // wave-uniform: the hits of these 64 entries, in entry (= term id) order
            const int src = __ffsll((long long)hb) - 1;
            hb &= hb - 1;
            const unsigned p = (unsigned)__builtin_amdgcn_readlane(packed, src);
            const int th = (int)(p >> 16);
            const float c = lex_contrib(idfs[th], (float)(p & 0xffffu), k1p1, norm);
            if ((mem[th] >> lane) & 1ull) {
              acc = acc + c;
              any = true;
            }
          }
        }
      }
      tile[(DW * w + dd) * TP + lane] = any ? acc : -1.0f;  // a document with no matching term: no candidate
    }
    __syncthreads();
    // ---- phase 2: the tile's 64 documents, one per lane, offered to this wave's QW query lists
    const int id = d0 + lane;
    const bool inr = id < n;
    unsigned mwd[QW];
#pragma unroll
    for (int j = 0; j < QW; ++j) mwd[j] = lex_mask_word(mk, mr[j], inr && w * QW + j < nq, id);
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const int q = w * QW + j;
      if (q < nq) {  // wave-uniform
        const float s = tile[lane * TP + q];
        const bool ok = inr && s >= 0.f && ((mwd[j] >> (id & 31)) & 1u);
        wave_offer(bv[j], bi[j], ok ? -s : FLT_MAX, ok ? id : -1, k, lane);
      }
    }
    __syncthreads();  // the tile is consumed before the next one is written
  }
#pragma unroll
  for (int j = 0; j < QW; ++j) {
    const int q = w * QW + j;
    if (q < nq && lane < k) {
      const size_t o = ((size_t)q * gridDim.x + blockIdx.x) * k + lane;
      out_v[o] = bv[j];
      out_i[o] = bi[j];
    }
  }
}

// in: [nq][G][k] sorted lists of (negated score, id) -> out: [nq][k] scores (fp32, descending) and ids (int64,
// ties -> lower id); missing results are (0, -1). One workgroup of LMW waves per query, each wave takes 64
// candidates (64 / k whole lists) per step; the waves' lists are merged last.
__global__ __launch_bounds__(LMW * 64) void lex_merge_kernel(const float* __restrict__ in_v,
                                                             const int* __restrict__ in_i, int G, int k,
                                                             float* __restrict__ out_s,
                                                             long long* __restrict__ out_i) {
  __shared__ float mv[LMW][64];
  __shared__ int mi[LMW][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qi = blockIdx.x;
  const int lpw = 64 / k;
  const int li = lane / k, e = lane % k;
  const size_t base = (size_t)qi * G * k;
  float bv = FLT_MAX;
  int bi = -1;
  for (int l0 = w * lpw; l0 < G; l0 += LMW * lpw) {  // wave-uniform
    const bool ok = li < lpw && l0 + li < G;
    const float v = ok ? in_v[base + (size_t)(l0 + li) * k + e] : FLT_MAX;
    const int id = ok ? in_i[base + (size_t)(l0 + li) * k + e] : -1;
    wave_offer(bv, bi, v, id, k, lane);
  }
  mv[w][lane] = bv;
  mi[w][lane] = bi;
  __syncthreads();
  if (w == 0) {
    for (int g = 1; g < LMW; ++g) wave_merge64(bv, bi, mv[g][lane], mi[g][lane], lane);
    if (lane < k) {
      out_s[(size_t)qi * k + lane] = bi >= 0 ? -bv : 0.f;
      out_i[(size_t)qi * k + lane] = bi;
    }
  }
}

}  // namespace

RAGK_API int ragk_lex_max_terms() { return LEX_TMAX; }

// Partial lists per query that ragk_lex_search emits for n documents (size the buffers [nq][G][k] with it).
RAGK_API int ragk_lex_search_groups(int n) {
  const int ntiles = (max(n, 0) + TILE - 1) / TILE;
  return max(1, min(ntiles, 1024));
}

// df[T] (int32) = number of live documents among the first n that hold qt[t]; qt sorted ascending, distinct.
// live: one bitmap row (bit doc & 31 of word doc >> 5) covering live_bits documents, or nullptr = all live.
RAGK_API int ragk_lex_df(const long long* row_ptr, const unsigned* terms, int n, const unsigned* qt, int T,
                         const unsigned* live, int live_bits, int* df, hipStream_t st) {
  if (T <= 0) return 0;
  if (T > LEX_TMAX || n < 0 || (live && live_bits < 0)) return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(df, 0, (size_t)T * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (n == 0) return 0;
  const int grid = max(1, min((n + 3) / 4, 1024));
  hipLaunchKernelGGL(lex_df_kernel, dim3(grid), dim3(LT), (size_t)T * 8, st, row_ptr, terms, n, qt, T, live,
                     live_bits, df);
  return (int)hipGetLastError();
}

// Top k (<= 64) documents per query for nq <= 64 queries. qt [T] sorted distinct term ids, idf [T], member [T]
// (bit q: query q holds the term). masks / qmask: optional per-query id bitmaps (LexMask). part_v / part_i hold
// nq * ragk_lex_search_groups(n) * k entries; results -> out_s / out_i [nq][k].
RAGK_API int ragk_lex_search(const long long* row_ptr, const unsigned* terms, const unsigned short* tf,
                             const int* doc_len, int n, const unsigned* qt, const float* idf,
                             const unsigned long long* member, int T, int nq, float k1, float k1p1, float b,
                             float avgdl, int k, const unsigned* masks, int mask_stride_words, int mask_bits,
                             const int* qmask, float* part_v, int* part_i, float* out_s, long long* out_i,
                             hipStream_t st) {
  if (nq <= 0) return 0;
  if (nq > 64 || k < 1 || k > 64 || T < 0 || T > LEX_TMAX || n < 0) return (int)hipErrorInvalidValue;
  if (qmask && !(mask_bits >= 0 && mask_stride_words >= 0 && (long long)mask_stride_words * 32 >= mask_bits &&
                 (masks || mask_bits == 0)))
    return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {  // up to 80 KiB of dynamic LDS needs the opt-in
    hipError_t e = hipFuncSetAttribute((const void*)lex_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       LEX_TMAX * 16 + TILE * TP * 4);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  const int ntiles = (n + TILE - 1) / TILE;
  const int G = ragk_lex_search_groups(n);
  const size_t lds = (size_t)T * 16 + (size_t)TILE * TP * 4;
  hipLaunchKernelGGL(lex_scan_kernel, dim3(G), dim3(LT), lds, st, row_ptr, terms, tf, doc_len, n, ntiles, qt, idf,
                     member, T, nq, k1, k1p1, b, avgdl, k, LexMask{masks, qmask, mask_stride_words, mask_bits},
                     part_v, part_i);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lex_merge_kernel, dim3(nq), dim3(LMW * 64), 0, st, part_v, part_i, G, k, out_s, out_i);
  return (int)hipGetLastError();
}
