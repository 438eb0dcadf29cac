// node2vec: biased second-order walks and the skip-gram fit on expected
// negatives (definition: n2v.h).
//
// n2v_walk_kernel: one lane per walk.  A walk is a chain of dependent loads
// (row bounds, the binary search in cum, the candidate, the binary search in
// the previous node's row), so there is nothing for a wave to share; the chains
// of 10 n walks hide each other's latency.  Every draw is keyed by (seed, step,
// try, walk position), so lanes diverge in their try counts without consequence.
//
// The skip-gram fit is the WEIGHT form of the two kernels of the logistic fits:
// sig_dense_kernel (sig_dense.h) for the dense term, sig_update_kernel
// (sig_update.h) for the sparse part and the AdaGrad step.
#include <cmath>

#include "n2v.h"
#include "philox.h"
#include "sig_update.h"

namespace ps {

constexpr int kN2vBlock = 256;
constexpr int kN2vTries = 256;

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
      const float beta = cand == prev ? A.inv_p : (row_holds(A.idx, pb, pe, (int32_t)cand) ? 1.f : A.inv_q);
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
  const SigUpdateArgs A{ptr, n_rows, {idx, val, 1.f, Y, nullptr, n_other, ldy, err}, X, nullptr, ldx, (int)f, D, ldd,
                        nullptr, rw, H, ldh, nullptr, reg, lr};
  sig_update_launch<true>(A, st);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
