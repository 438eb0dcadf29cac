// Logistic matrix factorisation, full-gradient AdaGrad ascent (definition: lmf.h).
//
// The dense term D = sigmoid(X Y^T + bx + by^T) Y and its row sums: the BIAS form
// of sig_dense_kernel (sig_dense.h), which describes the kernel.
//
// lmf_update_kernel: the sparse part and the AdaGrad step on the row plan of
// rowplan.h, one wave per row, the workgroup for a long row: the walk also
// gathers by[i] and carries the scalar sum of w_i, and wave 0 finishes a long row.
#include <algorithm>
#include <cmath>

#include "lmf.h"
#include "rowplan.h"
#include "sig_dense.h"

namespace ps {

constexpr float kLmfEps = 1e-6f;

struct LmfUpArgs {
  const int64_t* ptr;
  int64_t n_rows;
  RowItems I;
  float* X;
  float* bx;
  int64_t ldx;
  int f;
  const float* D;
  int64_t ldd;
  const float* dsum;
  float* H;
  int64_t ldh;
  float* hb;
  float reg, lr;
};

// LONG: called by every wave of the workgroup; barriers inside.
template <bool LONG>
__device__ __forceinline__ void lmf_row(const LmfUpArgs& A, int64_t row, float* __restrict__ part, int lane, int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float* hr = A.H + row * A.ldh + c0;
  const float2 x = row_ld2(xr, on);
  const float bxu = A.bx[row];
  // the sums over the row's items of w_i y_i, and of w_i
  float2 acc = make_float2(0.f, 0.f);
  float ws = 0.f;
  row_walk<true>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                 [&](float2 y, float cu, float bu) __attribute__((always_inline)) {
                   const float s = (wave_sum(fmaf(x.x, y.x, x.y * y.y)) + bxu) + bu;
                   const float w = cu * lmf_sigmoid(-s);
                   acc.x = fmaf(w, y.x, acc.x);
                   acc.y = fmaf(w, y.y, acc.y);
                   ws += w;
                 });
  if constexpr (LONG) {
    acc = row_wave_order_sum<false, true>(part, kRowMaxF, part + kRowWaves * kRowMaxF, lane, wv, c0, on, acc, ws);
    if (wv != 0) return;  // wave 0 has the sums and finishes the row
  }
  const float2 s = acc;
  if (on) {
    const float2 d = *reinterpret_cast<const float2*>(A.D + row * A.ldd + c0);
    float2 hh = *reinterpret_cast<const float2*>(hr);
    const float gx = fmaf(-A.reg, x.x, s.x - d.x), gy = fmaf(-A.reg, x.y, s.y - d.y);
    hh.x = fmaf(gx, gx, hh.x);
    hh.y = fmaf(gy, gy, hh.y);
    *reinterpret_cast<float2*>(hr) = hh;
    if (A.lr != 0.f)
      *reinterpret_cast<float2*>(xr) =
          make_float2(x.x + A.lr * gx / sqrtf(kLmfEps + hh.x), x.y + A.lr * gy / sqrtf(kLmfEps + hh.y));
  }
  if (lane == 0) {
    const float gb = ws - A.dsum[row];
    const float hn = fmaf(gb, gb, A.hb[row]);
    A.hb[row] = hn;
    if (A.lr != 0.f) A.bx[row] = bxu + A.lr * gb / sqrtf(kLmfEps + hn);
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void lmf_update_kernel(LmfUpArgs A) {
  __shared__ __attribute__((aligned(16))) float part[kRowWaves * kRowMaxF + kRowWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { lmf_row<false>(A, row, part, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { lmf_row<true>(A, row, part, lane, wv); });
}

int lmf_row_block() { return kSigRowBlock; }
int lmf_long_row() { return kRowLong; }

int launch_lmf_dense(const float* X, const float* bx, int64_t n_rows, int64_t ldx, const float* Y, const float* by,
                     int64_t n_other, int64_t ldy, int64_t f, float* D, int64_t ldd, float* dsum, hipStream_t st) {
  PS_TRY(row_tables_ok("lmf_dense", f, {{"X", X, ldx}, {"Y", Y, ldy}, {"D", D, ldd}}));
  PS_REQUIRE(bx != nullptr && by != nullptr && dsum != nullptr, kErrArg, "lmf_dense: null bias or dsum");
  PS_TRY(row_sizes_ok("lmf_dense", n_rows, n_other));
  if (n_rows == 0) return kOk;
  sig_dense_launch<false>(SigDenseArgs{X, bx, n_rows, ldx, Y, by, n_other, ldy, (int)f, D, ldd, dsum}, st);
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_lmf_update(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                      const float* by, int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f,
                      const float* D, int64_t ldd, const float* dsum, float* H, int64_t ldh, float* hb, float alpha,
                      float reg, float lr, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("lmf_update", f, {{"Y", Y, ldy}, {"X", X, ldx}, {"D", D, ldd}, {"H", H, ldh}}));
  PS_REQUIRE(ptr != nullptr && by != nullptr && bx != nullptr && dsum != nullptr && hb != nullptr, kErrArg,
             "lmf_update: null row pointers, bias, dsum or hb");
  PS_TRY(row_sizes_ok("lmf_update", n_rows, n_other));
  PS_REQUIRE(alpha > 0.f && alpha < INFINITY, kErrArg, "lmf_update: alpha must be positive and finite");
  PS_REQUIRE(reg >= 0.f && reg < INFINITY && lr >= 0.f && lr < INFINITY, kErrArg,
             "lmf_update: reg and lr must be non-negative and finite");
  if (n_rows == 0) return kOk;
  const LmfUpArgs A{ptr, n_rows, {idx, val, alpha, Y, by, n_other, ldy, err}, X, bx, ldx, (int)f, D, ldd, dsum, H, ldh,
                    hb, reg, lr};
  hipLaunchKernelGGL(lmf_update_kernel, dim3((unsigned)ceil_div(n_rows, kRowWaves)), dim3(64 * kRowWaves), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
