// Beyond-accuracy metrics over recommendation lists: the device work of
// eval.py:271-286 intra_diversity and :288-312 inter_diversity.
//
// Intra.  The reference gathers the K feature rows of each list and takes the
// mean of their K x K cosine matrix.  That mean is |sum_c f_c / |f_c||^2 / K^2
// (diagonal and repeated ids included), so per query it is a gather of K rows
// and one squared norm: HBM / Infinity-Cache bound, 4 bytes out per query.
// One wave per query (segment_wmean_kernel's shape): lanes own float4 column
// groups, kLmRows rows' loads are in flight per step, the sum runs in slot
// order per column, and the squares are added per lane in column order and
// across lanes by the xor butterfly: a fixed order, no atomics, the same bits
// on every run.
//
// Inter.  scipy's cosine distance between two one-hot rows is
// 1 - |A & B| / sqrt(|A| |B|) over the SETS of ids of the two lists, so a pair
// needs three integers.  Up to kOvBallot columns one wave compares all pairs
// of slots by ballot; longer lists are sorted in LDS by one workgroup, then
// deduplicated against the left neighbour and counted by binary search.
#include "listmetrics.h"

namespace ps {

constexpr int kLmWaves = 4;   // rows (row_inv_norm) / queries (list_intra_sim) per workgroup
constexpr int kLmRows = 8;    // feature rows whose loads are in flight per step
constexpr int kLmAcc = 2;     // column groups per lane: 128 (scalar) / 512 (float4) columns per pass
constexpr int kOvMaxK = 4096;  // list columns one pair may compare (LDS: 2 x 16 KiB)
constexpr int kOvBallot = 64;  // up to here one wave compares a pair by ballot
constexpr int kOvBlock = 256;

// ---------------------------------------------------------------- inverse row norms
// Plain IEEE sqrt and division (no v_rsq): a squared norm that is a power of
// four has an exact inverse.
template <bool VEC>
__global__ __launch_bounds__(64 * kLmWaves) void row_inv_norm_kernel(const float* __restrict__ x, int64_t n,
                                                                      int d, int64_t ld,
                                                                      float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kLmWaves + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* r = x + row * ld;
  float s = 0.f;
  if constexpr (VEC) {
    for (int c = 4 * lane; c < d; c += 256) {
      const float4 v = *reinterpret_cast<const float4*>(r + c);
      s = fmaf(v.x, v.x, s);
      s = fmaf(v.y, v.y, s);
      s = fmaf(v.z, v.z, s);
      s = fmaf(v.w, v.w, s);
    }
  } else {
    for (int c = lane; c < d; c += 64) s = fmaf(r[c], r[c], s);
  }
  s = wave_sum(s);
  if (lane == 0) inv[row] = __fdiv_rn(1.0f, __fsqrt_rn(s));
}

int launch_row_inv_norms(const float* x, int64_t n, int64_t d, int64_t ld, float* inv, hipStream_t st) {
  PS_REQUIRE(x != nullptr && inv != nullptr, kErrArg, "row_inv_norms: null pointer");
  PS_REQUIRE(n >= 0 && d >= 1 && ld >= d, kErrArg, "row_inv_norms: bad sizes (ld < d?)");
  PS_REQUIRE(n <= INT32_MAX && d <= INT32_MAX, kErrArg, "row_inv_norms: table too large");
  if (n == 0) return kOk;
  const bool vec = d % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const dim3 grid((unsigned)ceil_div(n, kLmWaves)), block(64 * kLmWaves);
  if (vec)
    hipLaunchKernelGGL(row_inv_norm_kernel<true>, grid, block, 0, st, x, n, (int)d, ld, inv);
  else
    hipLaunchKernelGGL(row_inv_norm_kernel<false>, grid, block, 0, st, x, n, (int)d, ld, inv);
  PS_CHECK_LAUNCH();
  return kOk;
}

// ---------------------------------------------------------------- intra-list similarity
// Wave i: s[col] = sum_{c < kc} inv[id_c] * feat[id_c][col] in slot order, then
// out[i] = (sum_col s[col]^2) / (float)(kc * kc).  A lane owns kLmAcc groups of
// W columns (W = 4: one float4) per pass; the column-pass loop repeats the list
// for d above 64 * W * kLmAcc columns.  The list is read 64 slots at a time
// (lane l: id and inv of slot j0 + l) and handed out by shuffle, so a row's
// base address is wave-uniform.  inf * 0 = NaN for a zero row is intended; a
// column group beyond d is never multiplied, so it stays out of the sum.
template <bool VEC>
__global__ __launch_bounds__(64 * kLmWaves) void list_intra_sim_kernel(
    const float* __restrict__ feat, int64_t n, int d, int64_t ld, const float* __restrict__ inv,
    const int64_t* __restrict__ lists, int64_t nq, int64_t ldk, int kc, float* __restrict__ out,
    int* __restrict__ err) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int kPass = 64 * W * kLmAcc;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kLmWaves + (threadIdx.x >> 6);
  if (i >= nq) return;  // wave-uniform
  const int64_t* li = lists + i * ldk;
  float sq = 0.f;
  for (int c0 = 0; c0 < d; c0 += kPass) {
    float acc[kLmAcc][W];
    int col[kLmAcc];   // the group's first column, 0 where the group lies beyond d (loaded, not used)
    bool on[kLmAcc];
#pragma unroll
    for (int a = 0; a < kLmAcc; ++a) {
      const int c = c0 + a * 64 * W + lane * W;
      on[a] = c < d;
      col[a] = on[a] ? c : 0;
#pragma unroll
      for (int e = 0; e < W; ++e) acc[a][e] = 0.f;
    }
    auto load = [&](const float* row, int a, float (&v)[W]) __attribute__((always_inline)) {
      if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(row + col[a]);
        v[0] = t.x;
        v[1] = t.y;
        v[2] = t.z;
        v[3] = t.w;
      } else {
        v[0] = row[col[a]];
      }
    };
    for (int j0 = 0; j0 < kc; j0 += 64) {
      const int m = min(64, kc - j0);
      long long id = 0;
      float w = 0.f;
      if (lane < m) {
        id = li[j0 + lane];
        if (id < 0 || id >= n) {  // callers validate; clamp so that no access strays
          if (err) atomicExch(err, 1);
          id = 0;
        }
        w = inv[id];
      }
      int u = 0;
      for (; u + kLmRows <= m; u += kLmRows) {
        float x[kLmRows][kLmAcc][W];
        float wu[kLmRows];
#pragma unroll
        for (int r = 0; r < kLmRows; ++r) {
          const float* row = feat + (int64_t)__shfl(id, u + r, 64) * ld;
          wu[r] = __shfl(w, u + r, 64);
#pragma unroll
          for (int a = 0; a < kLmAcc; ++a) load(row, a, x[r][a]);
        }
#pragma unroll
        for (int r = 0; r < kLmRows; ++r) {
#pragma unroll
          for (int a = 0; a < kLmAcc; ++a) {
#pragma unroll
            for (int e = 0; e < W; ++e) acc[a][e] = on[a] ? fmaf(wu[r], x[r][a][e], acc[a][e]) : acc[a][e];
          }
        }
      }
      for (; u < m; ++u) {
        const float* row = feat + (int64_t)__shfl(id, u, 64) * ld;
        const float w1 = __shfl(w, u, 64);
        float x[kLmAcc][W];
#pragma unroll
        for (int a = 0; a < kLmAcc; ++a) load(row, a, x[a]);
#pragma unroll
        for (int a = 0; a < kLmAcc; ++a) {
#pragma unroll
          for (int e = 0; e < W; ++e) acc[a][e] = on[a] ? fmaf(w1, x[a][e], acc[a][e]) : acc[a][e];
        }
      }
    }
#pragma unroll
    for (int a = 0; a < kLmAcc; ++a) {
#pragma unroll
      for (int e = 0; e < W; ++e) sq = on[a] ? fmaf(acc[a][e], acc[a][e], sq) : sq;
    }
  }
  sq = wave_sum(sq);
  if (lane == 0) out[i] = __fdiv_rn(sq, (float)((int64_t)kc * kc));
}

int launch_list_intra_sim(const float* feat, int64_t n, int64_t d, int64_t ld, const float* inv,
                          const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, float* out, int* err,
                          hipStream_t st) {
  PS_REQUIRE(feat != nullptr && inv != nullptr && lists != nullptr && out != nullptr, kErrArg,
             "list_intra_sim: null pointer");
  PS_REQUIRE(n >= 1 && d >= 1 && ld >= d && nq >= 0, kErrArg, "list_intra_sim: bad sizes (ld < d?)");
  PS_REQUIRE(kc >= 1 && kc <= ldk, kErrArg, "list_intra_sim: kc must be in [1, ldk]");
  PS_REQUIRE(n <= INT32_MAX && d <= INT32_MAX && kc <= (1 << 24), kErrArg, "list_intra_sim: too large");
  if (nq == 0) return kOk;
  PS_REQUIRE(nq <= (int64_t)INT32_MAX * kLmWaves, kErrArg, "list_intra_sim: too many queries");
  const bool vec = d % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0;
  const dim3 grid((unsigned)ceil_div(nq, kLmWaves)), block(64 * kLmWaves);
  if (vec)
    hipLaunchKernelGGL(list_intra_sim_kernel<true>, grid, block, 0, st, feat, n, (int)d, ld, inv, lists, nq, ldk,
                       (int)kc, out, err);
  else
    hipLaunchKernelGGL(list_intra_sim_kernel<false>, grid, block, 0, st, feat, n, (int)d, ld, inv, lists, nq, ldk,
                       (int)kc, out, err);
  PS_CHECK_LAUNCH();
  return kOk;
}

// ---------------------------------------------------------------- pair overlap
// a row index of `pairs` / an id of `lists`, clamped into range (callers validate)
__device__ __forceinline__ int64_t ov_clamp(int64_t v, int64_t bound, int* err) {
  if (v < 0 || v >= bound) {
    if (err) atomicExch(err, 1);
    v = 0;
  }
  return v;
}

// One wave per pair, kc <= 64: lane l holds slot l of both lists.  Slot c opens
// a new set member when no earlier slot holds its id (the first set bit of the
// ballot of equal slots is c itself); a new member of A is in the intersection
// when any slot of B holds it.  The counts are wave-uniform.
__global__ __launch_bounds__(64 * kLmWaves) void list_pair_overlap_ballot_kernel(
    const int64_t* __restrict__ lists, int64_t nq, int64_t ldk, int kc, int64_t n_ids,
    const int64_t* __restrict__ pairs, int64_t np, int32_t* __restrict__ out, int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kLmWaves + (threadIdx.x >> 6);
  if (p >= np) return;  // wave-uniform
  const int64_t a = ov_clamp(pairs[2 * p], nq, err), b = ov_clamp(pairs[2 * p + 1], nq, err);
  const bool on = lane < kc;
  const uint32_t va = on ? (uint32_t)ov_clamp(lists[a * ldk + lane], n_ids, err) : 0u;
  const uint32_t vb = on ? (uint32_t)ov_clamp(lists[b * ldk + lane], n_ids, err) : 0u;
  int na = 0, nb = 0, ni = 0;
  for (int c = 0; c < kc; ++c) {
    const uint32_t ac = __shfl(va, c, 64), bc = __shfl(vb, c, 64);
    const unsigned long long ma = __ballot(on && va == ac);
    const unsigned long long mb = __ballot(on && vb == bc);
    const unsigned long long mx = __ballot(on && vb == ac);
    if (__ffsll((long long)ma) - 1 == c) {
      ++na;
      if (mx != 0ull) ++ni;
    }
    if (__ffsll((long long)mb) - 1 == c) ++nb;
  }
  if (lane == 0) {
    out[3 * p] = na;
    out[3 * p + 1] = nb;
    out[3 * p + 2] = ni;
  }
}

// In-LDS bitonic sort, ascending, of two arrays of P (a power of two) ids at
// once (knn_bitonic's network).  All threads of the block call it.
__device__ void ov_bitonic2(uint32_t* x, uint32_t* y, int P) {
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < P; i += kOvBlock) {
        const int l = i ^ jj;
        if (l > i) {
          const bool up = (i & kk) == 0;
          const uint32_t xa = x[i], xb = x[l], ya = y[i], yb = y[l];
          if (up ? xa > xb : xa < xb) {
            x[i] = xb;
            x[l] = xa;
          }
          if (up ? ya > yb : ya < yb) {
            y[i] = yb;
            y[l] = ya;
          }
        }
      }
      __syncthreads();
    }
  }
}

// One workgroup per pair, 64 < kc <= kOvMaxK: both lists sorted in LDS (padded
// with 0xffffffff, above every id); slot i opens a new set member when it
// differs from its left neighbour, and a new member of A is searched in B.
__global__ __launch_bounds__(kOvBlock) void list_pair_overlap_sorted_kernel(
    const int64_t* __restrict__ lists, int64_t nq, int64_t ldk, int kc, int64_t n_ids,
    const int64_t* __restrict__ pairs, int64_t np, int32_t* __restrict__ out, int* __restrict__ err) {
  __shared__ uint32_t sa[kOvMaxK];
  __shared__ uint32_t sb[kOvMaxK];
  __shared__ int red[kOvBlock / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t p = blockIdx.x;
  const int64_t a = ov_clamp(pairs[2 * p], nq, err), b = ov_clamp(pairs[2 * p + 1], nq, err);
  int P = 2 * kOvBallot;
  while (P < kc) P <<= 1;  // kc <= kOvMaxK (the launcher refuses more): P <= kOvMaxK
  for (int i = tid; i < P; i += kOvBlock) {
    sa[i] = i < kc ? (uint32_t)ov_clamp(lists[a * ldk + i], n_ids, err) : 0xffffffffu;
    sb[i] = i < kc ? (uint32_t)ov_clamp(lists[b * ldk + i], n_ids, err) : 0xffffffffu;
  }
  __syncthreads();
  ov_bitonic2(sa, sb, P);
  int na = 0, nb = 0, ni = 0;
  for (int i = tid; i < kc; i += kOvBlock) {
    const uint32_t v = sa[i];
    if (i == 0 || sa[i - 1] != v) {
      ++na;
      int lo = 0, hi = kc;  // the first slot of B that is >= v
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sb[mid] < v) lo = mid + 1; else hi = mid;
      }
      if (lo < kc && sb[lo] == v) ++ni;
    }
    if (i == 0 || sb[i - 1] != sb[i]) ++nb;
  }
  na = wave_sum_i(na);
  nb = wave_sum_i(nb);
  ni = wave_sum_i(ni);
  if (lane == 0) {
    red[wv][0] = na;
    red[wv][1] = nb;
    red[wv][2] = ni;
  }
  __syncthreads();
  if (tid < 3) {
    int s = 0;
    for (int w = 0; w < kOvBlock / 64; ++w) s += red[w][tid];
    out[3 * p + tid] = s;
  }
}

int list_overlap_max_k() { return kOvMaxK; }

int launch_list_pair_overlap(const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, int64_t n_ids,
                             const int64_t* pairs, int64_t np, int32_t* out, int* err, hipStream_t st) {
  PS_REQUIRE(lists != nullptr && pairs != nullptr && out != nullptr, kErrArg, "list_pair_overlap: null pointer");
  PS_REQUIRE(nq >= 1 && np >= 0 && n_ids >= 1, kErrArg, "list_pair_overlap: bad sizes");
  PS_REQUIRE(kc >= 1 && kc <= ldk, kErrArg, "list_pair_overlap: kc must be in [1, ldk]");
  PS_REQUIRE(kc <= kOvMaxK, kErrArg, "list_pair_overlap: kc above pinsage_list_overlap_max_k() = 4096");
  PS_REQUIRE(n_ids <= INT32_MAX, kErrArg, "list_pair_overlap: ids must fit 32 bits (n_ids < 2^31)");
  PS_REQUIRE(np <= INT32_MAX, kErrArg, "list_pair_overlap: too many pairs");
  if (np == 0) return kOk;
  if (kc <= kOvBallot)
    hipLaunchKernelGGL(list_pair_overlap_ballot_kernel, dim3((unsigned)ceil_div(np, kLmWaves)), dim3(64 * kLmWaves),
                       0, st, lists, nq, ldk, (int)kc, n_ids, pairs, np, out, err);
  else
    hipLaunchKernelGGL(list_pair_overlap_sorted_kernel, dim3((unsigned)np), dim3(kOvBlock), 0, st, lists, nq, ldk,
                       (int)kc, n_ids, pairs, np, out, err);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
