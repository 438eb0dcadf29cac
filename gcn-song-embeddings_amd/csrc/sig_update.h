// sig_update_kernel: the sparse part and the AdaGrad step of the full-gradient
// logistic fits on the row plan of rowplan.h, one wave per row, the workgroup
// for a long row (wave 0 finishes it), after sig_dense_kernel has left D:
//   BIAS form   (lmf.hip):  s_i = x.y_i + bx + by_i,  g = sum_i w_i y_i - D - reg x,
//     and the scalar sum of w_i is carried for gb = sum_i w_i - dsum, with which
//     lane 0 steps bx and hb
//   WEIGHT form (n2v.hip):  s_i = x.y_i,  g = sum_i w_i y_i - rw D - reg x, rw a weight per row
// with w_i = alpha val_i sigmoid(-s_i) over the row's items, then h += g^2 and
// x += lr g / sqrt(eps + h); lr == 0 leaves x (and bx) unwritten.  The two forms
// differ in the score, in the factor on D and in the bias step, nowhere else.
#pragma once
#include "sig_dense.h"

namespace ps {

constexpr float kSigEps = 1e-6f;

// WEIGHT form: rw is the row weight; I.by, bx, dsum and hb are unused (null).  BIAS form: rw is unused
struct SigUpdateArgs {
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
  const float* rw;
  float* H;
  int64_t ldh;
  float* hb;
  float reg, lr;
};

// LONG: called by every wave of the workgroup; barriers inside.
template <bool WEIGHT, bool LONG>
__device__ __forceinline__ void sig_update_row(const SigUpdateArgs& A, int64_t row, float* __restrict__ part, int lane,
                                               int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float* hr = A.H + row * A.ldh + c0;
  const float2 x = row_ld2(xr, on);
  float bxu = 0.f;
  if constexpr (!WEIGHT) bxu = A.bx[row];
  // the sums over the row's items of w_i y_i, and (BIAS) of w_i
  float2 acc = make_float2(0.f, 0.f);
  float ws = 0.f;
  row_walk<!WEIGHT>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                    [&](float2 y, float cu, float bu) __attribute__((always_inline)) {
                      float s = wave_sum(fmaf(x.x, y.x, x.y * y.y));
                      if constexpr (!WEIGHT) s = (s + bxu) + bu;
                      const float w = cu * lmf_sigmoid(-s);
                      acc.x = fmaf(w, y.x, acc.x);
                      acc.y = fmaf(w, y.y, acc.y);
                      if constexpr (!WEIGHT) ws += w;
                    });
  if constexpr (LONG) {
    acc = row_wave_order_sum<false, !WEIGHT>(part, kRowMaxF, part + kRowWaves * kRowMaxF, lane, wv, c0, on, acc, ws);
    if (wv != 0) return;  // wave 0 has the sums and finishes the row
  }
  if (on) {
    // BIAS: fmaf(-1, d, acc) rounds once, as acc - d does
    float nrw = -1.f;
    if constexpr (WEIGHT) nrw = -A.rw[row];
    const float2 d = *reinterpret_cast<const float2*>(A.D + row * A.ldd + c0);
    float2 hh = *reinterpret_cast<const float2*>(hr);
    const float gx = fmaf(-A.reg, x.x, fmaf(nrw, d.x, acc.x)), gy = fmaf(-A.reg, x.y, fmaf(nrw, d.y, acc.y));
    hh.x = fmaf(gx, gx, hh.x);
    hh.y = fmaf(gy, gy, hh.y);
    *reinterpret_cast<float2*>(hr) = hh;
    if (A.lr != 0.f)
      *reinterpret_cast<float2*>(xr) =
          make_float2(x.x + A.lr * gx / sqrtf(kSigEps + hh.x), x.y + A.lr * gy / sqrtf(kSigEps + hh.y));
  }
  if constexpr (!WEIGHT)
    if (lane == 0) {
      const float gb = ws - A.dsum[row];
      const float hn = fmaf(gb, gb, A.hb[row]);
      A.hb[row] = hn;
      if (A.lr != 0.f) A.bx[row] = bxu + A.lr * gb / sqrtf(kSigEps + hn);
    }
}

template <bool WEIGHT>
__global__ __launch_bounds__(64 * kRowWaves) void sig_update_kernel(SigUpdateArgs A) {
  // the long row's partial sums, and behind them (BIAS) the waves' scalar sums
  __shared__ __attribute__((aligned(16))) float part[kRowWaves * kRowMaxF + (WEIGHT ? 0 : kRowWaves)];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { sig_update_row<WEIGHT, false>(A, row, part, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { sig_update_row<WEIGHT, true>(A, row, part, lane, wv); });
}

template <bool WEIGHT>
inline void sig_update_launch(const SigUpdateArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(sig_update_kernel<WEIGHT>, dim3((unsigned)ceil_div(A.n_rows, kRowWaves)), dim3(64 * kRowWaves), 0,
                     st, A);
}

}  // namespace ps
