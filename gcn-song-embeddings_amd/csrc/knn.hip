// Cosine k-nearest neighbours over an embedding table (the evaluation path
// that consumes PinSage embeddings: baselines.py:69-77 cosine_sim_ab and
// :91-103 knn_from_emb, called by eval.py:112-143 save_knn with k = 1000).
//
//   sim(q, j) = dot(e_q, e_j) / (|e_q| |e_j| + eps)      (fp32, as torch.mm / torch.norm)
//   out[q]    = the k largest sim(q, .) over all rows j, sorted descending
//
// Per batch of query rows: one fp32 MFMA GEMM (launch_gemm: gathered query
// rows x the whole table, K = d) writes the dot products to HBM, then one
// workgroup per query row selects its top k: a threshold from the row's first
// 4096 keys (LDS radix select), ONE pass that keeps every key >= it in per-wave
// LDS segments, a radix select of the k-th key among those candidates, and an
// LDS bitonic sort of the keys >= it.  Rows where that cannot be exact (fewer
// than k candidates, a full segment) take the original path: an MSB-first
// radix select over the whole row on the order-preserving uint32 image of the
// similarity (12 + 12 + 8 bit digits, histograms in LDS), then the same sort.  Exact ties at the
// k-th key keep the lowest column indices; the final order is (sim desc,
// index asc).  The row of dot products stays in the Infinity Cache across the
// select's four passes when the batch is sized to it.
//
// The selection kernel is a template over a key policy (what a row holds and
// how a key is made of it): cosine over dot products here, Jaccard over the
// co-occurrence counts of cooc.hip (launch_knn_select_jaccard), finished scores
// over its weighted sums (launch_knn_select_score).
//
// The ranks of given rows in that order (the positives of held-out pairs:
// eval.py:227-250 hit_rate / mrr) are counted without any list by
// rank_count_kernel at the end of this file, over the same dot products,
// norms and key function.
#include <algorithm>

#include "gemm.h"
#include "knn.h"

namespace ps {

constexpr int kKnnBlock = 1024;
constexpr int kKnnMaxK = 4096;

__device__ __forceinline__ uint32_t f2key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// The key every kernel here orders by: the image of dot / (|q| |e_j| + eps),
// (|q| |e_j| + eps) rounded like torch's rank-1 mm then add: no contraction
__device__ __forceinline__ uint32_t knn_key(float dot, float na, float nj, float eps) {
  return f2key(dot / __fadd_rn(__fmul_rn(na, nj), eps));
}

// What knn_select_kernel orders a row by.  A policy names the row's element
// type, the per-column array it is paired with and the per-row scalar, and turns
// one (row value, column value, row scalar) into a key.  kFloor: no key is below
// kFloorKey (a row may consist almost wholly of it).
struct KnnCosineKey {  // row of dot products, norms[], |q|
  using Row = float;
  using Row4 = float4;
  using Col = float;
  using Col4 = float4;
  using Scalar = float;
  static constexpr bool kFloor = false;
  static constexpr uint32_t kFloorKey = 0u;
  float eps;
  __device__ __forceinline__ uint32_t operator()(float dot, float nj, float na) const {
    return knn_key(dot, na, nj, eps);
  }
};
// Jaccard similarity of two tracks' collection sets (baselines.py:211-217):
// row of co-occurrence counts, deg[], deg[q];  co / (union + 1e-10) as torch
// computes it over int32 tensors and a Python float: the union is rounded to
// fp32, 1e-10 vanishes unless the union is 0, IEEE division.
struct KnnJaccardKey {
  using Row = int32_t;
  using Row4 = int4;
  using Col = int32_t;
  using Col4 = int4;
  using Scalar = int32_t;
  static constexpr bool kFloor = true;
  static constexpr uint32_t kFloorKey = 0x80000000u;  // f2key(0.0f): scores are >= 0
  __device__ __forceinline__ uint32_t operator()(int32_t co, int32_t dj, int32_t dq) const {
    return f2key((float)co / __fadd_rn((float)(dq + dj - co), 1e-10f));
  }
};
// A row of finished scores >= 0 (the weighted sums of cooc.hip as floats): the
// key is the score's own image; the column value and the row scalar take no part.
struct KnnScoreKey {
  using Row = float;
  using Row4 = float4;
  using Col = float;
  using Col4 = float4;
  using Scalar = float;
  static constexpr bool kFloor = true;
  static constexpr uint32_t kFloorKey = 0x80000000u;  // f2key(0.0f)
  __device__ __forceinline__ uint32_t operator()(float s, float, float) const { return f2key(s); }
};

__global__ void knn_row_norms_kernel(const float* __restrict__ e, int64_t n, int d, int64_t ld,
                                     float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= n) return;
  const float* r = e + row * ld;
  // torch.norm on CPU accumulates float rows in double (acc_type<float> = double)
  double s = 0.0;
  for (int c = lane; c < d; c += 64) s += (double)r[c] * (double)r[c];
  s = wave_sum_d(s);
  if (lane == 0) norms[row] = (float)sqrt(s);
}

__global__ void knn_ids_kernel(const int64_t* __restrict__ q, int64_t nq, int64_t n,
                               int32_t* __restrict__ q32, float* __restrict__ qn,
                               const float* __restrict__ norms, int* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  int64_t v = q[i];
  if (v < 0 || v >= n) {  // callers validate; clamp so that no access strays
    if (err) atomicExch(err, 1);
    v = 0;
  }
  q32[i] = (int32_t)v;
  qn[i] = norms[v];
}

// one workgroup per query row b: dots[b][0..n) -> top k of sim, sorted
constexpr int kKnnSample = 4096;  // leading keys of a row that set the candidate threshold
constexpr int kKnnSeg = 512;      // candidate slots per wave (16 waves: 8192 per row)

// In-LDS bitonic sort of P (a power of two) (key, index) pairs into the final
// order: key descending, then index ascending.  All threads of the block call it.
__device__ void knn_bitonic(uint32_t* key, int32_t* idx, int P) {
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < P; i += kKnnBlock) {
        const int l = i ^ jj;
        if (l > i) {
          const uint32_t ka = key[i], kb = key[l];
          const int32_t ia = idx[i], ib = idx[l];
          const bool a_first = ka > kb || (ka == kb && ia < ib);
          const bool up = (i & kk) == 0;
          if (up ? !a_first : a_first) {
            key[i] = kb;
            key[l] = ka;
            idx[i] = ib;
            idx[l] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
}

// The rank-th largest of keys held in LDS (12 + 12 + 8 bit MSB-first radix
// select; `get(i)` reads key i of `cnt`): returns it, and in *need_eq how
// many keys equal to it are within the top `rank`.  All threads call it.
template <class Get>
__device__ uint32_t knn_lds_kth(Get get, int cnt, uint32_t rank, uint32_t* hist, uint32_t* sh,
                                uint32_t* need_eq) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t prefix = 0, need = rank;
  const int shifts[3] = {20, 8, 0};
  const int widths[3] = {12, 12, 8};
#pragma unroll 1
  for (int p = 0; p < 3; ++p) {
    const int sh_ = shifts[p], nb = 1 << widths[p], hs = sh_ + widths[p];
    for (int i = tid; i < nb; i += kKnnBlock) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < cnt; i += kKnnBlock) {
      const uint32_t key = get(i);
      if (hs >= 32 || (key >> hs) == prefix) atomicAdd(&hist[(key >> sh_) & (nb - 1)], 1u);
    }
    __syncthreads();
    if (wv == 0) {
      const int per = nb / 64;
      uint32_t s = 0;
      for (int i = 0; i < per; ++i) s += hist[nb - 1 - (lane * per + i)];
      uint32_t inc = s;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      const uint32_t before = inc - s;
      if (before < need && need <= inc) {
        uint32_t c = before;
        for (int i = 0; i < per; ++i) {
          const int bin = nb - 1 - (lane * per + i);
          const uint32_t h = hist[bin];
          if (c + h >= need) {
            sh[0] = (prefix << widths[p]) | (uint32_t)bin;
            sh[1] = need - c;
            break;
          }
          c += h;
        }
      }
    }
    __syncthreads();
    prefix = sh[0];
    need = sh[1];
    __syncthreads();
  }
  *need_eq = need;
  return prefix;
}

template <class KP>
__global__ __launch_bounds__(kKnnBlock) void knn_select_kernel(
    const typename KP::Row* __restrict__ dots, int64_t n, const typename KP::Col* __restrict__ norms,
    const typename KP::Scalar* __restrict__ qn, KP kp, int k, int P, float* __restrict__ out_w,
    int64_t* __restrict__ out_n) {
  using Row = typename KP::Row;
  using Col = typename KP::Col;
  using Row4 = typename KP::Row4;
  using Col4 = typename KP::Col4;
  __shared__ uint32_t hist[4096];
  __shared__ uint32_t skey[kKnnMaxK];
  __shared__ int32_t sidx[kKnnMaxK];
  __shared__ uint32_t sh_prefix, sh_need;
  __shared__ int sh_gt, sh_eq;
  __shared__ int wave_cnt[kKnnBlock / 64];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const Row* row = dots + b * n;
  const typename KP::Scalar na = qn[b];
  auto key_of = [&](Row dot, Col nj) __attribute__((always_inline)) { return kp(dot, nj, na); };
  auto key_at = [&](int64_t j) __attribute__((always_inline)) { return key_of(row[j], norms[j]); };
  // rows of n % 4 == 0 elements start 16-byte aligned (the rows are n apart)
  const bool vec = (n % 4) == 0;

  // ---- one pass.  A threshold t = a key of the row's leading kKnnSample keys
  // whose rank there lies (with wide slack) below k's expected rank; one pass
  // keeps every key >= t in per-wave LDS segments (no shared counter).  If at
  // least k keys reach t, the k-th largest key does too, so the candidates hold
  // the whole top k and its ties: a radix select over them gives the k-th key,
  // and sorting the keys >= it gives the exact result.  Otherwise (too few,
  // a full segment, or more than kKnnMaxK keys >= the k-th) the 4-pass radix
  // select below runs.
  __shared__ uint32_t ckey[16 * kKnnSeg];
  __shared__ int32_t cidx[16 * kKnnSeg];
  __shared__ int seg_cnt[kKnnBlock / 64];
  __shared__ uint32_t sh2[2];
  {
    const int S = (int)min<int64_t>(n, kKnnSample);
    for (int i = tid; i < S; i += kKnnBlock) skey[i] = key_at(i);
    __syncthreads();
    const double er = (double)k * S / (double)n;
    const uint32_t r = S == n ? (uint32_t)k : (uint32_t)min<double>(S, er * 1.5 + 4.0 * sqrt(er) + 8.0);
    uint32_t dummy;
    const uint32_t t = knn_lds_kth([&](int i) { return skey[i]; }, S, r, hist, sh2, &dummy);
    // a floor threshold over more keys than the segments hold: every key passes
    // it and some segment overflows, so the pass visits nothing and reports a
    // full segment (block-uniform; never taken by a policy without a floor)
    const bool doomed = KP::kFloor && t == KP::kFloorKey && n > 16 * kKnnSeg;
    const int64_t np = doomed ? 0 : n;
    int cw = 0;  // this wave's candidates (wave-uniform)
    bool over = false;
    uint32_t* const wk = ckey + wv * kKnnSeg;
    int32_t* const wi = cidx + wv * kKnnSeg;
    auto take = [&](uint32_t key, int64_t j, bool valid) __attribute__((always_inline)) {
      const bool c = valid && key >= t;
      const unsigned long long m = __ballot(c);
      if (c) {
        const int slot = cw + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < kKnnSeg) {
          wk[slot] = key;
          wi[slot] = (int32_t)j;
        }
      }
      cw += __popcll(m);
    };
    // block-uniform trip counts: take() uses wave-wide ballots
    const int64_t n16 = vec ? (np / 16) * 16 : 0;
    for (int64_t base = 0; base < n16; base += (int64_t)kKnnBlock * 16) {
      const int64_t j0 = base + (int64_t)tid * 16;
      const bool ok = j0 < n16;
      const int64_t jl = ok ? j0 : 0;
      Row4 dv[4];
      Col4 nv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dv[u] = *reinterpret_cast<const Row4*>(row + jl + 4 * u);
        nv[u] = *reinterpret_cast<const Col4*>(norms + jl + 4 * u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        take(key_of(dv[u].x, nv[u].x), j0 + 4 * u, ok);
        take(key_of(dv[u].y, nv[u].y), j0 + 4 * u + 1, ok);
        take(key_of(dv[u].z, nv[u].z), j0 + 4 * u + 2, ok);
        take(key_of(dv[u].w, nv[u].w), j0 + 4 * u + 3, ok);
      }
    }
    for (int64_t j0 = n16; j0 < np; j0 += kKnnBlock) {
      const int64_t j = j0 + tid;
      take(j < np ? key_at(j) : 0u, j, j < np);
    }
    over = doomed || cw > kKnnSeg;
    if (lane == 0) seg_cnt[wv] = over ? -1 : cw;
    __syncthreads();
    int tot = 0;
    bool bad = false;
    for (int w = 0; w < kKnnBlock / 64; ++w) {
      bad |= seg_cnt[w] < 0;
      tot += seg_cnt[w] < 0 ? 0 : seg_cnt[w];
    }
    if (!bad && tot >= k) {
      // candidate i (0 <= i < 16 * kKnnSeg) lives in segment i / kKnnSeg
      auto cand = [&](int i) -> uint32_t {
        const int w = i / kKnnSeg, o = i - w * kKnnSeg;
        return o < seg_cnt[w] ? ckey[i] : 0u;  // key 0 sorts below every real key
      };
      uint32_t need_eq;
      const uint32_t thr = knn_lds_kth(cand, 16 * kKnnSeg, (uint32_t)k, hist, sh2, &need_eq);
      // keys >= thr: the n_gt keys above it plus every tie
      if (tid == 0) sh_gt = 0;
      __syncthreads();
      for (int i0 = 0; i0 < 16 * kKnnSeg; i0 += kKnnBlock) {  // block-uniform: ballots below
        const int i = i0 + tid, w = i / kKnnSeg, o = i - w * kKnnSeg;
        const bool c = o < seg_cnt[w] && ckey[i] >= thr;
        const unsigned long long mm = __ballot(c);
        int base = 0;
        if (lane == 0 && mm) base = atomicAdd(&sh_gt, __popcll(mm));
        base = __shfl(base, 0, 64);
        const int sl = base + __popcll(mm & ((1ull << lane) - 1ull));
        if (c && sl < kKnnMaxK) {
          skey[sl] = ckey[i];
          sidx[sl] = cidx[i];
        }
      }
      __syncthreads();
      const int m = sh_gt;
      if (m <= kKnnMaxK) {
        int PC = 64;
        while (PC < m) PC <<= 1;
        for (int i = m + tid; i < PC; i += kKnnBlock) {
          skey[i] = 0u;
          sidx[i] = 0x7fffffff;
        }
        __syncthreads();
        knn_bitonic(skey, sidx, PC);
        for (int i = tid; i < k; i += kKnnBlock) {
          out_w[b * k + i] = key2f(skey[i]);
          out_n[b * k + i] = sidx[i];
        }
        return;  // block-uniform (m is a shared value read after a barrier)
      }
    }
    __syncthreads();
  }

  // ---- radix select of the k-th largest key: digits of 12, 12 and 8 bits
  uint32_t prefix = 0, need = (uint32_t)k;
  const int shifts[3] = {20, 8, 0};
  const int widths[3] = {12, 12, 8};
#pragma unroll 1
  for (int p = 0; p < 3; ++p) {
    const int sh = shifts[p], nb = 1 << widths[p];
    for (int i = tid; i < nb; i += kKnnBlock) hist[i] = 0;
    __syncthreads();
    const int hs = sh + widths[p];  // bits above this digit must equal the prefix
    // keys at the policy's floor (most of a sparse row: one bin) are counted in
    // a register and added once per thread
    uint32_t n_floor = 0;
    auto count = [&](uint32_t key) __attribute__((always_inline)) {
      if (KP::kFloor && key == KP::kFloorKey) {
        ++n_floor;
        return;
      }
      if (hs >= 32 || (key >> hs) == prefix) atomicAdd(&hist[(key >> sh) & (nb - 1)], 1u);
    };
    // 4 x 16-byte loads of dots and norms in flight per thread (the row is
    // streamed four times: memory-level parallelism, not LDS, bounds a pass)
    const int64_t n16 = vec ? (n / 16) * 16 : 0;
    for (int64_t j0 = (int64_t)tid * 16; j0 < n16; j0 += (int64_t)kKnnBlock * 16) {
      Row4 dv[4];
      Col4 nv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dv[u] = *reinterpret_cast<const Row4*>(row + j0 + 4 * u);
        nv[u] = *reinterpret_cast<const Col4*>(norms + j0 + 4 * u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        count(key_of(dv[u].x, nv[u].x));
        count(key_of(dv[u].y, nv[u].y));
        count(key_of(dv[u].z, nv[u].z));
        count(key_of(dv[u].w, nv[u].w));
      }
    }
    for (int64_t j = n16 + tid; j < n; j += kKnnBlock) count(key_at(j));
    if (KP::kFloor && n_floor && (hs >= 32 || (KP::kFloorKey >> hs) == prefix))
      atomicAdd(&hist[(KP::kFloorKey >> sh) & (nb - 1)], n_floor);
    __syncthreads();
    if (wv == 0) {  // scan bins from the top: the bin holding the need-th largest
      const int per = nb / 64;
      uint32_t s = 0;
      for (int i = 0; i < per; ++i) s += hist[nb - 1 - (lane * per + i)];
      // exclusive prefix over lanes (lane 0 = highest bins)
      uint32_t inc = s;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      const uint32_t before = inc - s;
      if (before < need && need <= inc) {  // exactly one lane
        uint32_t c = before;
        for (int i = 0; i < per; ++i) {
          const int bin = nb - 1 - (lane * per + i);
          const uint32_t h = hist[bin];
          if (c + h >= need) {
            sh_prefix = (prefix << widths[p]) | (uint32_t)bin;
            sh_need = need - c;
            break;
          }
          c += h;
        }
      }
    }
    __syncthreads();
    prefix = sh_prefix;
    need = sh_need;
    __syncthreads();
  }
  const uint32_t thr = prefix;        // the k-th largest key
  const int need_eq = (int)need;      // how many keys == thr belong to the top k
  const int n_gt = k - need_eq;

  // ---- collect: keys > thr (any order) and the lowest-index need_eq keys == thr
  if (tid == 0) {
    sh_gt = 0;
    sh_eq = 0;
  }
  __syncthreads();
  for (int64_t j0 = 0; j0 < n; j0 += kKnnBlock) {
    const int64_t j = j0 + tid;
    uint32_t key = 0;
    bool gt = false, eq = false;
    if (j < n) {
      key = key_at(j);
      gt = key > thr;
      eq = key == thr;
    }
    if (gt) {
      const int s = atomicAdd(&sh_gt, 1);
      skey[s] = key;
      sidx[s] = (int32_t)j;
    }
    // ordered compaction of the ties (index order within and across chunks)
    const unsigned long long m = __ballot(eq);
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    const int taken = sh_eq;
    if (eq) {
      int r = taken + __popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wv; ++w) r += wave_cnt[w];
      if (r < need_eq) {
        skey[n_gt + r] = key;
        sidx[n_gt + r] = (int32_t)j;
      }
    }
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < kKnnBlock / 64; ++w) t += wave_cnt[w];
      sh_eq = taken + t;
    }
    __syncthreads();
    if (sh_eq >= need_eq && sh_gt >= n_gt) break;  // uniform: shared values after a barrier
  }
  // ---- sort (key desc, index asc); pad to P with keys that sort last
  for (int i = k + tid; i < P; i += kKnnBlock) {
    skey[i] = 0u;
    sidx[i] = 0x7fffffff;
  }
  __syncthreads();
  knn_bitonic(skey, sidx, P);
  for (int i = tid; i < k; i += kKnnBlock) {
    out_w[b * k + i] = key2f(skey[i]);
    out_n[b * k + i] = sidx[i];
  }
}

int64_t knn_scratch_bytes(int64_t n, int64_t qb) {
  return align_up(n * 4, 256) + align_up(qb * 4, 256) * 2 + align_up(qb * n * 4, 256) + 256;
}

int launch_knn_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries,
                      int64_t nq, int64_t k, float eps, void* scratch, int64_t scratch_bytes,
                      float* out_w, int64_t* out_n, int* err, hipStream_t st) {
  PS_REQUIRE(n > 0 && d > 0 && ld >= d && nq >= 0, kErrArg, "knn: bad sizes");
  PS_REQUIRE(d % 4 == 0, kErrArg, "knn: d must be a multiple of 4");
  // the GEMM reads rows in 16-byte pieces straight into LDS: every row starts aligned
  PS_REQUIRE(ld % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0, kErrArg,
             "knn: ld must be a multiple of 4 and emb 16-byte aligned");
  PS_REQUIRE(n <= INT32_MAX && d <= INT32_MAX, kErrArg, "knn: table too large");
  PS_REQUIRE(k >= 1 && k <= n && k <= kKnnMaxK, kErrArg, "knn: need 1 <= k <= min(n, 4096)");
  if (nq == 0) return kOk;
  // batch of query rows that fits the scratch
  int64_t qb = std::min<int64_t>(nq, 65535);
  qb = std::min<int64_t>(qb, std::max<int64_t>(1, (scratch_bytes - align_up(n * 4, 256) - 1024) /
                                                     (n * 4 + 8)));
  while (qb > 1 && knn_scratch_bytes(n, qb) > scratch_bytes) --qb;
  PS_REQUIRE(knn_scratch_bytes(n, qb) <= scratch_bytes, kErrWorkspace, "knn: scratch too small");
  char* s = (char*)scratch;
  float* norms = (float*)s;
  s += align_up(n * 4, 256);
  int32_t* q32 = (int32_t*)s;
  s += align_up(qb * 4, 256);
  float* qn = (float*)s;
  s += align_up(qb * 4, 256);
  float* dots = (float*)s;

  hipLaunchKernelGGL(knn_row_norms_kernel, dim3((unsigned)ceil_div(n * 64, 256)), dim3(256), 0, st,
                     emb, n, (int)d, ld, norms);
  PS_CHECK_LAUNCH();
  int P = 64;
  while (P < k) P <<= 1;
  for (int64_t q0 = 0; q0 < nq; q0 += qb) {
    const int64_t m = std::min(qb, nq - q0);
    hipLaunchKernelGGL(knn_ids_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st,
                       queries + q0, m, n, q32, qn, norms, err);
    PS_CHECK_LAUNCH();
    GemmParams p;
    p.M = (int)m;
    p.N = (int)n;
    p.K = (int)d;
    p.a = emb;
    p.lda = ld;
    p.a_idx = q32;
    p.b = emb;
    p.ldb = ld;
    p.c = dots;
    p.ldc = n;
    PS_TRY(launch_gemm(p, st));
    hipLaunchKernelGGL(knn_select_kernel<KnnCosineKey>, dim3((unsigned)m), dim3(kKnnBlock), 0, st, dots, n,
                       norms, qn, KnnCosineKey{eps}, (int)k, P, out_w + q0 * k, out_n + q0 * k);
    PS_CHECK_LAUNCH();
  }
  return kOk;
}

int knn_max_k() { return kKnnMaxK; }

int launch_knn_select_jaccard(const int32_t* counts, int64_t n, const int32_t* deg, const int32_t* qdeg, int64_t m,
                              int64_t k, float* out_w, int64_t* out_n, hipStream_t st) {
  PS_REQUIRE(n > 0 && n <= INT32_MAX && m >= 0 && m <= 65535, kErrArg, "knn: bad sizes");
  PS_REQUIRE(k >= 1 && k <= n && k <= kKnnMaxK, kErrArg, "knn: need 1 <= k <= min(n, 4096)");
  if (m == 0) return kOk;
  int P = 64;
  while (P < k) P <<= 1;
  hipLaunchKernelGGL(knn_select_kernel<KnnJaccardKey>, dim3((unsigned)m), dim3(kKnnBlock), 0, st, counts, n, deg,
                     qdeg, KnnJaccardKey{}, (int)k, P, out_w, out_n);
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_knn_select_score(const float* scores, int64_t n, int64_t m, int64_t k, float* out_w, int64_t* out_n,
                            hipStream_t st) {
  PS_REQUIRE(n > 0 && n <= INT32_MAX && m >= 0 && m <= 65535, kErrArg, "knn: bad sizes");
  PS_REQUIRE(k >= 1 && k <= n && k <= kKnnMaxK, kErrArg, "knn: need 1 <= k <= min(n, 4096)");
  if (m == 0) return kOk;
  int P = 64;
  while (P < k) P <<= 1;
  // the policy reads neither the per-column array nor the row scalar, but the
  // kernel's text loads both: the first score row (n floats, aligned as a row)
  // and the first m <= m * n scores are valid memory for them
  hipLaunchKernelGGL(knn_select_kernel<KnnScoreKey>, dim3((unsigned)m), dim3(kKnnBlock), 0, st, scores, n, scores,
                     scores, KnnScoreKey{}, (int)k, P, out_w, out_n);
  PS_CHECK_LAUNCH();
  return kOk;
}

// ---------------------------------------------------------------- ranks of given rows
// The rank of target row t for query q: how many rows j come before t in the
// order above (key descending, index ascending).  hit_rate and mrr (eval.py:
// 227-250) are functions of that one integer per (q, pos) pair, so neither
// needs a list.  One workgroup per query row streams the row's keys ONCE and
// ranks all m targets of its group in that pass:
//   m <= kRankFew: the targets' (key, index) words sit in registers, each is
//     counted by ballot + popcount into wave-private counts, combined in LDS;
//   otherwise: the group is sorted best-first in LDS (knn_bitonic), each j
//     binary-searches the first target it comes before and adds 1 to that slot
//     of an LDS histogram; the inclusive prefix over the slots is the ranks.
// Every count is an integer add: the result does not depend on the order.
constexpr int kRankMaxGroup = 4096;  // targets of one query row (LDS: keys, ids, histogram)
constexpr int kRankFew = 8;          // up to here the targets are held in registers

// (key, index) as one integer: j comes before t exactly when word(j) > word(t)
__device__ __forceinline__ uint64_t rank_word(uint32_t key, int32_t j) {
  return ((uint64_t)key << 32) | (uint32_t)(0x7fffffff - j);
}

// visit(key, j, valid) over the keys of one row, every thread the same number
// of times (visit may use wave-wide ballots): 4 x 16-byte loads of dots and
// norms per thread where n % 4 == 0, the scalar path otherwise and for the tail.
template <class Visit>
__device__ __forceinline__ void rank_stream(const float* __restrict__ row, const float* __restrict__ norms,
                                            int64_t n, float na, float eps, Visit visit) {
  const int tid = threadIdx.x;
  const int64_t n16 = (n % 4) == 0 ? (n / 16) * 16 : 0;
  for (int64_t base = 0; base < n16; base += (int64_t)kKnnBlock * 16) {
    const int64_t j0 = base + (int64_t)tid * 16;
    const bool ok = j0 < n16;
    const int64_t jl = ok ? j0 : 0;
    float4 dv[4], nv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dv[u] = *reinterpret_cast<const float4*>(row + jl + 4 * u);
      nv[u] = *reinterpret_cast<const float4*>(norms + jl + 4 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      visit(knn_key(dv[u].x, na, nv[u].x, eps), j0 + 4 * u, ok);
      visit(knn_key(dv[u].y, na, nv[u].y, eps), j0 + 4 * u + 1, ok);
      visit(knn_key(dv[u].z, na, nv[u].z, eps), j0 + 4 * u + 2, ok);
      visit(knn_key(dv[u].w, na, nv[u].w, eps), j0 + 4 * u + 3, ok);
    }
  }
  for (int64_t j0 = n16; j0 < n; j0 += kKnnBlock) {
    const int64_t j = j0 + tid;
    const bool ok = j < n;
    visit(ok ? knn_key(row[j], na, norms[j], eps) : 0u, j, ok);
  }
}

// first i in [0, m) with pred(i), or m: pred is false ... false true ... true
template <class Pred>
__device__ __forceinline__ int rank_first(int m, Pred pred) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pred(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kKnnBlock) void rank_count_kernel(
    const float* __restrict__ dots, int64_t n, const float* __restrict__ norms,
    const float* __restrict__ qn, float eps, const int64_t* __restrict__ grp_ptr,
    const int64_t* __restrict__ targets, int64_t* __restrict__ out_rank, int* __restrict__ err) {
  __shared__ uint32_t skey[kRankMaxGroup];
  __shared__ int32_t sidx[kRankMaxGroup];
  __shared__ int hist[kRankMaxGroup];
  __shared__ int wsum[kKnnBlock / 64][kRankFew];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* row = dots + b * n;
  const float na = qn[b];
  const int64_t g0 = grp_ptr[b];
  const int m = (int)(grp_ptr[b + 1] - g0);  // <= kRankMaxGroup (the launcher refuses more)
  if (m <= 0) return;                        // block-uniform
  auto target = [&](int i) {
    int64_t t = targets[g0 + i];
    if (t < 0 || t >= n) {  // callers validate; clamp so that no access strays
      if (err) atomicExch(err, 1);
      t = 0;
    }
    return (int32_t)t;
  };
  for (int i = tid; i < m; i += kKnnBlock) {
    const int32_t t = target(i);
    skey[i] = knn_key(row[t], na, norms[t], eps);
    sidx[i] = t;
  }
  __syncthreads();

  if (m <= kRankFew) {
    uint64_t tw[kRankFew];
    int cnt[kRankFew];  // wave-uniform
#pragma unroll
    for (int i = 0; i < kRankFew; ++i) {
      tw[i] = i < m ? rank_word(skey[i], sidx[i]) : ~0ull;  // no word is above ~0
      cnt[i] = 0;
    }
    rank_stream(row, norms, n, na, eps, [&](uint32_t key, int64_t j, bool valid) __attribute__((always_inline)) {
      const uint64_t w = rank_word(key, (int32_t)j);
#pragma unroll
      for (int i = 0; i < kRankFew; ++i) cnt[i] += __popcll(__ballot(valid && w > tw[i]));
    });
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kRankFew; ++i) wsum[wv][i] = cnt[i];
    }
    __syncthreads();
    if (tid < m) {
      int r = 0;
      for (int w = 0; w < kKnnBlock / 64; ++w) r += wsum[w][tid];
      out_rank[g0 + tid] = r;
    }
    return;
  }

  // ---- sorted form: slots in the final order, one histogram add per j
  int P = 64;
  while (P < m) P <<= 1;
  for (int i = m + tid; i < P; i += kKnnBlock) {
    skey[i] = 0u;
    sidx[i] = 0x7fffffff;
  }
  for (int i = tid; i < m; i += kKnnBlock) hist[i] = 0;
  __syncthreads();
  knn_bitonic(skey, sidx, P);
  rank_stream(row, norms, n, na, eps, [&](uint32_t key, int64_t j, bool valid) __attribute__((always_inline)) {
    // the first target j comes before; j then comes before every later one too
    const int s = !valid ? m : rank_first(m, [&](int i) {
      const uint32_t sk = skey[i];
      return key > sk || (key == sk && (int32_t)j < sidx[i]);
    });
    // a wave whose rows mostly share one slot (all below, or all above, the
    // group) adds to it once, not 64 times on one address
    const unsigned long long act = __ballot(s < m);
    if (act) {
      const int s0 = __shfl(s, __ffsll((long long)act) - 1, 64);
      const unsigned long long same = __ballot(s == s0);
      if (s == s0) {
        if ((same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&hist[s0], __popcll(same));
      } else if (s < m) {
        atomicAdd(&hist[s], 1);
      }
    }
  });
  __syncthreads();
  // inclusive prefix over the m slots, in place: thread tid owns slots 4 tid .. 4 tid + 3
  {
    int v[4], s = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = 4 * tid + c;
      v[c] = i < m ? hist[i] : 0;
      s += v[c];
    }
    int inc = s;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wsum[wv][0] = inc;
    __syncthreads();
    int run = inc - s;
    for (int w = 0; w < wv; ++w) run += wsum[w][0];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = 4 * tid + c;
      run += v[c];
      if (i < m) hist[i] = run;
    }
  }
  __syncthreads();
  // back to the caller's order: a target finds its own slot (a target listed
  // twice holds two equal slots; either one carries the same prefix)
  for (int i = tid; i < m; i += kKnnBlock) {
    const int32_t t = target(i);
    const uint32_t key = knn_key(row[t], na, norms[t], eps);
    const int s = rank_first(m, [&](int c) {
      const uint32_t sk = skey[c];
      return !(sk > key || (sk == key && sidx[c] < t));
    });
    out_rank[g0 + i] = hist[s];
  }
}

int64_t rank_scratch_bytes(int64_t n, int64_t qb) {
  return knn_scratch_bytes(n, qb) + align_up((qb + 1) * 8, 256);
}

int rank_max_group() { return kRankMaxGroup; }

int launch_rank_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries,
                       int64_t nu, const int64_t* grp_ptr, const int64_t* targets, int64_t np, float eps,
                       void* scratch, int64_t scratch_bytes, int64_t* out_rank, int* err, hipStream_t st) {
  PS_REQUIRE(n > 0 && d > 0 && ld >= d && nu >= 0 && np >= 0, kErrArg, "rank: bad sizes");
  PS_REQUIRE(d % 4 == 0, kErrArg, "rank: d must be a multiple of 4");
  PS_REQUIRE(ld % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0, kErrArg,
             "rank: ld must be a multiple of 4 and emb 16-byte aligned");
  PS_REQUIRE(n <= INT32_MAX && d <= INT32_MAX, kErrArg, "rank: table too large");
  PS_REQUIRE(grp_ptr != nullptr && grp_ptr[0] == 0, kErrArg, "rank: grp_ptr must start at 0");
  for (int64_t u = 0; u < nu; ++u) {
    const int64_t m = grp_ptr[u + 1] - grp_ptr[u];
    PS_REQUIRE(m >= 0, kErrArg, "rank: grp_ptr must not decrease");
    PS_REQUIRE(m <= kRankMaxGroup, kErrArg, "rank: a group holds more than 4096 targets (repeat the query row)");
  }
  PS_REQUIRE(grp_ptr[nu] == np, kErrArg, "rank: grp_ptr must end at the number of pairs");
  if (nu == 0) return kOk;
  // batch of query rows that fits the scratch
  // (a row costs at least n * 4 + 16 bytes: start one above that bound and step down)
  int64_t qb = std::min<int64_t>(nu, 65535);
  qb = std::min<int64_t>(qb, std::max<int64_t>(1, (scratch_bytes - align_up(n * 4, 256)) / (n * 4 + 16) + 1));
  while (qb > 1 && rank_scratch_bytes(n, qb) > scratch_bytes) --qb;
  PS_REQUIRE(rank_scratch_bytes(n, qb) <= scratch_bytes, kErrWorkspace, "rank: scratch too small");
  char* s = (char*)scratch;
  float* norms = (float*)s;
  s += align_up(n * 4, 256);
  int32_t* q32 = (int32_t*)s;
  s += align_up(qb * 4, 256);
  float* qn = (float*)s;
  s += align_up(qb * 4, 256);
  int64_t* gp = (int64_t*)s;
  s += align_up((qb + 1) * 8, 256);
  float* dots = (float*)s;

  hipLaunchKernelGGL(knn_row_norms_kernel, dim3((unsigned)ceil_div(n * 64, 256)), dim3(256), 0, st,
                     emb, n, (int)d, ld, norms);
  PS_CHECK_LAUNCH();
  for (int64_t q0 = 0; q0 < nu; q0 += qb) {
    const int64_t m = std::min(qb, nu - q0);
    // the batch's slice of grp_ptr (absolute offsets into targets / out_rank)
    PS_CHECK_HIP(hipMemcpyAsync(gp, grp_ptr + q0, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(knn_ids_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st,
                       queries + q0, m, n, q32, qn, norms, err);
    PS_CHECK_LAUNCH();
    GemmParams p;
    p.M = (int)m;
    p.N = (int)n;
    p.K = (int)d;
    p.a = emb;
    p.lda = ld;
    p.a_idx = q32;
    p.b = emb;
    p.ldb = ld;
    p.c = dots;
    p.ldc = n;
    PS_TRY(launch_gemm(p, st));
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)m), dim3(kKnnBlock), 0, st, dots, n, norms, qn, eps,
                       gp, targets, out_rank, err);
    PS_CHECK_LAUNCH();
  }
  return kOk;
}

}  // namespace ps
