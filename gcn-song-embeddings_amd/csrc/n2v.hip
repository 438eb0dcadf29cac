// node2vec: biased second-order walks and the skip-gram fit on expected
// negatives (definition: n2v.h).
//
// n2v_walk_kernel: one lane per walk.  A walk is a chain of dependent loads
// (row bounds, the binary search in cum, the candidate, the binary search in
// the previous node's row), so there is nothing for a wave to share; the chains
// of 10 n walks hide each other's latency.  Every draw is keyed by (seed, step,
// try, walk position), so lanes diverge in their try counts without consequence.
//
// The dense term is the WEIGHT form of sig_dense_kernel (sig_dense.h).
// sgns_update_kernel: the sparse part and the AdaGrad step on the row plan of
// rowplan.h, as lmf_update_kernel without biases and with the row weight on D.
#include <cmath>

#include "n2v.h"
#include "philox.h"
#include "rowplan.h"
#include "sig_dense.h"

namespace ps {

constexpr int kN2vBlock = 256;
constexpr int kN2vTries = 256;
constexpr float kSgnsEps = 1e-6f;

struct N2vArgs {
  const int64_t* ptr;
  const int32_t* idx;
  const int64_t* cum;
  int64_t n_nodes;
  const int64_t* starts;
  int64_t n_walks;
  int length;
  float inv_p, inv_q, M;
  uint64_t seed;
  uint32_t offset;
  int64_t walk_base;
  int32_t* walks;
  int* err;
};

// whether node v is in the ascending row [b, e) of idx
__device__ __forceinline__ bool n2v_in_row(const int32_t* __restrict__ idx, int64_t b, int64_t e, int32_t v) {
  while (b < e) {
    const int64_t m = b + ((e - b) >> 1);
    const int32_t a = idx[m];
    if (a == v) return true;
    if (a < v) b = m + 1;
    else e = m;
  }
  return false;
}

__global__ __launch_bounds__(kN2vBlock) void n2v_walk_kernel(N2vArgs A) {
  const int64_t k = (int64_t)blockIdx.x * kN2vBlock + threadIdx.x;
  if (k >= A.n_walks) return;
  int32_t* w = A.walks + k * A.length;
  const uint64_t pos = (uint64_t)(A.walk_base + k);
  int64_t cur = A.starts[k];
  if (cur < 0 || cur >= A.n_nodes) {  // callers validate; clamp so that no access strays
    if (A.err) atomicExch(A.err, 1);
    cur = 0;
  }
  w[0] = (int32_t)cur;
  int64_t prev = -1, pb = 0, pe = 0;  // the previous node and its row
  int j = 1;
  for (; j < A.length; ++j) {
    const int64_t b = A.ptr[cur], e = A.ptr[cur + 1];
    if (e <= b) break;  // no edges: the walk ends
    const uint64_t total = A.cum ? (uint64_t)A.cum[e - 1] : (uint64_t)(e - b);
    int64_t cand = 0;
    for (int t = 0; t < kN2vTries; ++t) {
      const uint4 r = philox10(A.seed, make_uint4((uint32_t)j * 256u + (uint32_t)t, (uint32_t)pos,
                                                  (uint32_t)(pos >> 32), A.offset));
      const uint64_t pick = __umul64hi((uint64_t)r.x | ((uint64_t)r.y << 32), total);
      int64_t edge;
      if (A.cum) {  // the first edge whose cum exceeds pick; the last edge's does, so lo stays inside the row
        int64_t lo = b, hi = e - 1;
        while (lo < hi) {
          const int64_t m = lo + ((hi - lo) >> 1);
          if ((uint64_t)A.cum[m] > pick) hi = m;
          else lo = m + 1;
        }
        edge = lo;
      } else {
        edge = b + (int64_t)pick;  // pick < total = e - b
      }
      cand = A.idx[edge];
      if (cand < 0 || cand >= A.n_nodes) {
        if (A.err) atomicExch(A.err, 1);
        cand = 0;
      }
      if (j == 1) break;
      const float beta = cand == prev ? A.inv_p : (n2v_in_row(A.idx, pb, pe, (int32_t)cand) ? 1.f : A.inv_q);
      const float u = (float)(r.z >> 8) * 0x1p-24f;  // exact
      if (u * A.M < beta) break;
    }
    prev = cur;
    pb = b;
    pe = e;
    cur = cand;
    w[j] = (int32_t)cand;
  }
  for (; j < A.length; ++j) w[j] = -1;
}

int launch_n2v_walk(const int64_t* ptr, const int32_t* idx, const int64_t* cum, int64_t n_nodes,
                    const int64_t* starts, int64_t n_walks, int64_t length, float inv_p, float inv_q, uint64_t seed,
                    uint32_t offset, int64_t walk_base, int32_t* walks, int* err, hipStream_t st) {
  PS_REQUIRE(inv_p > 0.f && inv_p < INFINITY && inv_q > 0.f && inv_q < INFINITY, kErrArg,
             "n2v_walk: 1/p and 1/q must be positive and finite");
  const float hi = fmaxf(fmaxf(inv_p, inv_q), 1.f), lo = fminf(fminf(inv_p, inv_q), 1.f);
  PS_REQUIRE(hi / lo <= 16.f, kErrArg, "n2v_walk: max(1/p, 1, 1/q) / min(1/p, 1, 1/q) must not exceed 16");
  PS_REQUIRE(length >= 1 && length < (1 << 24), kErrArg, "n2v_walk: need 1 <= length < 2^24");
  PS_REQUIRE(n_nodes >= 1 && n_nodes <= INT32_MAX && n_walks >= 0 && n_walks <= INT32_MAX && walk_base >= 0,
             kErrArg, "n2v_walk: bad sizes");
  PS_REQUIRE(ptr != nullptr && idx != nullptr, kErrArg, "n2v_walk: null graph");
  if (n_walks == 0) return kOk;
  PS_REQUIRE(starts != nullptr && walks != nullptr, kErrArg, "n2v_walk: null starts or walks");
  const N2vArgs A{ptr, idx, cum, n_nodes, starts, n_walks, (int)length, inv_p, inv_q, hi, seed, offset, walk_base,
                  walks, err};
  hipLaunchKernelGGL(n2v_walk_kernel, dim3((unsigned)ceil_div(n_walks, kN2vBlock)), dim3(kN2vBlock), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_sgns_dense(const float* X, int64_t n_rows, int64_t ldx, const float* Y, const float* cw, int64_t n_other,
                      int64_t ldy, int64_t f, float* D, int64_t ldd, hipStream_t st) {
  PS_TRY(row_tables_ok("sgns_dense", f, {{"X", X, ldx}, {"Y", Y, ldy}, {"D", D, ldd}}));
  PS_REQUIRE(cw != nullptr, kErrArg, "sgns_dense: null column weights");
  PS_TRY(row_sizes_ok("sgns_dense", n_rows, n_other));
  if (n_rows == 0) return kOk;
  sig_dense_launch<true>(SigDenseArgs{X, nullptr, n_rows, ldx, Y, cw, n_other, ldy, (int)f, D, ldd, nullptr}, st);
  PS_CHECK_LAUNCH();
  return kOk;
}

struct SgnsUpArgs {
  const int64_t* ptr;
  const float* rw;
  int64_t n_rows;
  RowItems I;
  float* X;
  int64_t ldx;
  int f;
  const float* D;
  int64_t ldd;
  float* H;
  int64_t ldh;
  float reg, lr;
};

// LONG: called by every wave of the workgroup; barriers inside.
template <bool LONG>
__device__ __forceinline__ void sgns_row(const SgnsUpArgs& A, int64_t row, float* __restrict__ part, int lane,
                                         int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float* hr = A.H + row * A.ldh + c0;
  const float2 x = row_ld2(xr, on);
  // the sum over the row's items of w_i y_i
  float2 acc = make_float2(0.f, 0.f);
  row_walk<false>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                  [&](float2 y, float cu, float) __attribute__((always_inline)) {
                    const float s = wave_sum(fmaf(x.x, y.x, x.y * y.y));
                    const float w = cu * lmf_sigmoid(-s);
                    acc.x = fmaf(w, y.x, acc.x);
                    acc.y = fmaf(w, y.y, acc.y);
                  });
  if constexpr (LONG) {
    float none = 0.f;
    acc = row_wave_order_sum<false, false>(part, kRowMaxF, nullptr, lane, wv, c0, on, acc, none);
    if (wv != 0) return;  // wave 0 has the sums and finishes the row
  }
  if (on) {
    const float nrw = -A.rw[row];
    const float2 d = *reinterpret_cast<const float2*>(A.D + row * A.ldd + c0);
    float2 hh = *reinterpret_cast<const float2*>(hr);
    const float gx = fmaf(-A.reg, x.x, fmaf(nrw, d.x, acc.x)), gy = fmaf(-A.reg, x.y, fmaf(nrw, d.y, acc.y));
    hh.x = fmaf(gx, gx, hh.x);
    hh.y = fmaf(gy, gy, hh.y);
    *reinterpret_cast<float2*>(hr) = hh;
    if (A.lr != 0.f)
      *reinterpret_cast<float2*>(xr) =
          make_float2(x.x + A.lr * gx / sqrtf(kSgnsEps + hh.x), x.y + A.lr * gy / sqrtf(kSgnsEps + hh.y));
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void sgns_update_kernel(SgnsUpArgs A) {
  __shared__ __attribute__((aligned(16))) float part[kRowWaves * kRowMaxF];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { sgns_row<false>(A, row, part, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { sgns_row<true>(A, row, part, lane, wv); });
}

int launch_sgns_update(const int64_t* ptr, const int32_t* idx, const float* val, const float* rw, int64_t n_rows,
                       const float* Y, int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* D,
                       int64_t ldd, float* H, int64_t ldh, float reg, float lr, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("sgns_update", f, {{"Y", Y, ldy}, {"X", X, ldx}, {"D", D, ldd}, {"H", H, ldh}}));
  PS_REQUIRE(ptr != nullptr && rw != nullptr, kErrArg, "sgns_update: null row pointers or row weights");
  PS_TRY(row_sizes_ok("sgns_update", n_rows, n_other));
  PS_REQUIRE(reg >= 0.f && reg < INFINITY && lr >= 0.f && lr < INFINITY, kErrArg,
             "sgns_update: reg and lr must be non-negative and finite");
  if (n_rows == 0) return kOk;
  // alpha = 1: the walk's weight is 1.f * val, exactly val
  const SgnsUpArgs A{ptr, rw, n_rows, {idx, val, 1.f, Y, nullptr, n_other, ldy, err}, X, ldx, (int)f, D, ldd, H, ldh,
                     reg, lr};
  hipLaunchKernelGGL(sgns_update_kernel, dim3((unsigned)ceil_div(n_rows, kRowWaves)), dim3(64 * kRowWaves), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
