// Bayesian personalised ranking: Philox negatives and the Jacobi AdaGrad
// half-iteration (definition: bpr.h), both on the row plan of rowplan.h.
//
// bpr_sample_kernel: a row's samples in groups of 64.  The draw is a chain of
// dependent integer steps (Philox, the binary search in the row), so a lane
// takes a sample and lanes diverge in their try counts without consequence;
// the two dots of a sample are the wave's, two columns per lane, the 64 samples
// of the group one after another with the loads of four of them in flight.
//
// bpr_apply_kernel: row_walk's gather with a signed weight per entry, the long
// row's partial sums in wave order, then the AdaGrad step of sig_update_kernel
// without a dense term.
#include <cmath>

#include "bpr.h"
#include "philox.h"
#include "sig_update.h"

namespace ps {

constexpr int kBprTries = 16;
constexpr int kBprMaxNeg = 8;
constexpr int kBprInFlight = 4;  // samples (two rows of Y each) whose loads are in flight per step

int bpr_max_tries() { return kBprTries; }

struct BprSampleArgs {
  const int64_t* ptr;
  const int32_t* idx;
  int64_t n_rows, cell_base;
  const float* X;
  int64_t ldx;
  const float* Y;
  const float* by;
  int64_t n_other, ldy;
  int f, S;
  uint64_t seed;
  uint32_t round16, offset;  // round16 = rho * 16: try k is counter word round16 + k
  int32_t* neg;
  float* w;
  int* err;
};

template <bool LONG>
__device__ __forceinline__ void bpr_sample_row(const BprSampleArgs& A, int64_t row, int lane, int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  const int64_t ns = (e - b) * A.S;  // the row's samples: q = (cell - b) S + s
  const float2 x = row_ld2(A.X + row * A.ldx + c0, on);
  const int64_t q_first = LONG ? wv * 64 : 0, q_step = LONG ? kRowWaves * 64 : 64;
  for (int64_t q0 = q_first; q0 < ns; q0 += q_step) {  // wave-uniform
    const int m = (int)min<int64_t>(64, ns - q0);
    int i = 0, j = 0, jn = -1;  // a void sample's second dot reads row 0 and is dropped
    float bi = 0.f, bj = 0.f;
    if (lane < m) {
      const int64_t q = q0 + lane;
      i = A.idx[b + q / A.S];
      if (i < 0 || i >= A.n_other) {  // callers validate; clamp so that no access strays
        if (A.err) atomicExch(A.err, 1);
        i = 0;
      }
      const uint64_t t = (uint64_t)((A.cell_base + b) * A.S + q);
      for (int k = 0; k < kBprTries; ++k) {
        const uint4 r =
            philox10(A.seed, make_uint4(A.round16 + (uint32_t)k, (uint32_t)t, (uint32_t)(t >> 32), A.offset));
        const int32_t cand = (int32_t)__umulhi(r.x, (uint32_t)A.n_other);  // < n_other
        if (!row_holds(A.idx, b, e, cand)) {
          jn = cand;
          break;
        }
      }
      bi = A.by[i];
      if (jn >= 0) {
        j = jn;
        bj = A.by[j];
      }
    }
    float sp = 0.f, sn = 0.f;
    auto dots = [&](int u, float2 yi, float2 yj) __attribute__((always_inline)) {
      const float si = wave_sum(fmaf(x.x, yi.x, x.y * yi.y)), sj = wave_sum(fmaf(x.x, yj.x, x.y * yj.y));
      if (lane == u) {
        sp = si;
        sn = sj;
      }
    };
    int u = 0;
    for (; u + kBprInFlight <= m; u += kBprInFlight) {
      float2 yi[kBprInFlight], yj[kBprInFlight];
#pragma unroll
      for (int r = 0; r < kBprInFlight; ++r) {
        yi[r] = row_ld2(A.Y + (int64_t)__shfl(i, u + r, 64) * A.ldy + c0, on);
        yj[r] = row_ld2(A.Y + (int64_t)__shfl(j, u + r, 64) * A.ldy + c0, on);
      }
#pragma unroll
      for (int r = 0; r < kBprInFlight; ++r) dots(u + r, yi[r], yj[r]);
    }
    for (; u < m; ++u)
      dots(u, row_ld2(A.Y + (int64_t)__shfl(i, u, 64) * A.ldy + c0, on),
           row_ld2(A.Y + (int64_t)__shfl(j, u, 64) * A.ldy + c0, on));
    if (lane < m) {
      const int64_t o = b * A.S + q0 + lane;  // < ptr[n_rows] S
      const float z = (sp + bi) - (sn + bj);
      A.neg[o] = jn;
      A.w[o] = jn >= 0 ? lmf_sigmoid(-z) : 0.f;
    }
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void bpr_sample_kernel(BprSampleArgs A) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { bpr_sample_row<false>(A, row, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { bpr_sample_row<true>(A, row, lane, wv); });
}

int launch_bpr_sample(const int64_t* ptr, const int32_t* idx, int64_t n_rows, int64_t cell_base, const float* X,
                      int64_t ldx, const float* Y, const float* by, int64_t n_other, int64_t ldy, int64_t f, int64_t S,
                      uint64_t seed, int64_t rho, uint32_t offset, int32_t* neg, float* w, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("bpr_sample", f, {{"X", X, ldx}, {"Y", Y, ldy}}));
  PS_REQUIRE(ptr != nullptr && by != nullptr, kErrArg, "bpr_sample: null row pointers or bias");
  PS_TRY(row_sizes_ok("bpr_sample", n_rows, n_other));
  PS_REQUIRE(S >= 1 && S <= kBprMaxNeg, kErrArg, "bpr_sample: need 1 <= negatives <= 8");
  PS_REQUIRE(rho >= 0 && rho < (1 << 27), kErrArg, "bpr_sample: need 0 <= rho < 2^27");
  PS_REQUIRE(cell_base >= 0, kErrArg, "bpr_sample: negative cell_base");
  if (n_rows == 0) return kOk;
  const BprSampleArgs A{ptr, idx, n_rows, cell_base, X, ldx, Y, by, n_other, ldy, (int)f, (int)S, seed,
                        (uint32_t)rho * 16u, offset, neg, w, err};
  hipLaunchKernelGGL(bpr_sample_kernel, dim3((unsigned)ceil_div(n_rows, kRowWaves)), dim3(64 * kRowWaves), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

// bx and hb are null together: a half without a bias
struct BprApplyArgs {
  const int64_t* ptr;
  int64_t n_rows;
  RowItems I;
  float* X;
  float* bx;
  int64_t ldx;
  int f;
  float* H;
  int64_t ldh;
  float* hb;
  float reg, lr;
};

// LONG: called by every wave of the workgroup; barriers inside.
template <bool LONG>
__device__ __forceinline__ void bpr_apply_row(const BprApplyArgs& A, int64_t row, float* __restrict__ part, int lane,
                                              int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float* hr = A.H + row * A.ldh + c0;
  const float2 x = row_ld2(xr, on);
  // the sums over the row's entries of val_e y_e, and of val_e
  float2 acc = make_float2(0.f, 0.f);
  float sv = 0.f;
  row_walk<false>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                  [&](float2 y, float cu, float) __attribute__((always_inline)) {
                    acc.x = fmaf(cu, y.x, acc.x);
                    acc.y = fmaf(cu, y.y, acc.y);
                    sv += cu;
                  });
  if constexpr (LONG) {
    acc = row_wave_order_sum<false, true>(part, kRowMaxF, part + kRowWaves * kRowMaxF, lane, wv, c0, on, acc, sv);
    if (wv != 0) return;  // wave 0 has the sums and finishes the row
  }
  if (on) {
    float2 hh = *reinterpret_cast<const float2*>(hr);
    const float gx = fmaf(-A.reg, x.x, acc.x), gy = fmaf(-A.reg, x.y, acc.y);
    hh.x = fmaf(gx, gx, hh.x);
    hh.y = fmaf(gy, gy, hh.y);
    *reinterpret_cast<float2*>(hr) = hh;
    if (A.lr != 0.f)
      *reinterpret_cast<float2*>(xr) =
          make_float2(x.x + A.lr * gx / sqrtf(kSigEps + hh.x), x.y + A.lr * gy / sqrtf(kSigEps + hh.y));
  }
  if (A.bx != nullptr && lane == 0) {
    const float hn = fmaf(sv, sv, A.hb[row]);
    A.hb[row] = hn;
    if (A.lr != 0.f) A.bx[row] = A.bx[row] + A.lr * sv / sqrtf(kSigEps + hn);
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void bpr_apply_kernel(BprApplyArgs A) {
  // the long row's partial sums, and behind them the waves' scalar sums
  __shared__ __attribute__((aligned(16))) float part[kRowWaves * kRowMaxF + kRowWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { bpr_apply_row<false>(A, row, part, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { bpr_apply_row<true>(A, row, part, lane, wv); });
}

int launch_bpr_apply(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                     int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f, float* H, int64_t ldh,
                     float* hb, float reg, float lr, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("bpr_apply", f, {{"Y", Y, ldy}, {"X", X, ldx}, {"H", H, ldh}}));
  PS_REQUIRE(ptr != nullptr, kErrArg, "bpr_apply: null row pointers");
  PS_REQUIRE((bx == nullptr) == (hb == nullptr), kErrArg, "bpr_apply: bx and hb must both be given or both be null");
  PS_TRY(row_sizes_ok("bpr_apply", n_rows, n_other));
  PS_REQUIRE(reg >= 0.f && reg < INFINITY && lr >= 0.f && lr < INFINITY, kErrArg,
             "bpr_apply: reg and lr must be non-negative and finite");
  if (n_rows == 0) return kOk;
  // alpha = 1: the entry's weight is 1.f * val, exactly val
  const BprApplyArgs A{ptr, n_rows, {idx, val, 1.f, Y, nullptr, n_other, ldy, err}, X, bx, ldx, (int)f, H, ldh, hb,
                       reg, lr};
  hipLaunchKernelGGL(bpr_apply_kernel, dim3((unsigned)ceil_div(n_rows, kRowWaves)), dim3(64 * kRowWaves), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
