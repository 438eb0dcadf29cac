// Logistic matrix factorisation (Johnson 2014), full-gradient AdaGrad ascent:
// the dense sigmoid(X Y^T) Y term and the rest of one half-iteration (lmf.hip).
//
// The model (this project's definition; no parity with a package is claimed):
// R [n_users, n_items] is a CSR with values r > 0, c = alpha r.  Tables X
// [n_users, f], Y [n_items, f], biases bx, by;  s_ui = x_u . y_i + bx_u + by_i.
// The objective to maximise is
//   L = sum_obs c s - sum_obs (1 + c) softplus(s) - sum_unobs softplus(s)
//       - (reg / 2)(|X|^2 + |Y|^2)                      (biases not regularised)
// One iteration updates every user row from (Y, by), then every item row from
// the new (X, bx) with R^T as the CSR.  A half-iteration is Jacobi.  Per row u,
// in fp32:
//   D    = sum_all i sig(s_ui) y_i         dsum = sum_all i sig(s_ui)
//   w_i  = c_ui sig(-s_ui)  for observed i
//   g    = sum_obs w_i y_i - D - reg x_u   gb = sum_obs w_i - dsum
//   h   += g^2 (elementwise)               hb += gb^2     (AdaGrad, start at 0)
//   x_u += lr g / sqrt(1e-6 + h)           bx_u += lr gb / sqrt(1e-6 + hb)
// sig is evaluated stably: for s >= 0 it is 1 / (1 + e^-s), otherwise
// e^s / (1 + e^s); never NaN or Inf for finite s.
#pragma once
#include "common.h"

namespace ps {

// rows of X that one workgroup of launch_lmf_dense owns
int lmf_row_block();
// a row with more items than this is taken by a whole workgroup of
// launch_lmf_update, its item sums split over the waves and added in wave
// order; at most this many: one wave
int lmf_long_row();

// D f32 [n_rows][ldd] (columns [0, f)) and dsum f32 [n_rows] as defined above,
// for every row of X f32 [n_rows][ldx], bx f32 [n_rows] against all of Y f32
// [n_other][ldy], by f32 [n_other].  Fused: the scores exist in registers only.
// Exact-f32 MFMA for both products; a workgroup owns lmf_row_block() rows and
// walks all items in ascending order, so there is no cross-workgroup reduction
// and no atomic: the same bits on every run, and the bits of row u depend on
// x_u, bx_u, Y, by only.  Columns [f, ld) of no table are read or written.
// Needs 4 <= f <= 128, f % 4 == 0, every ld >= f and % 4 == 0, X, Y, D 16-byte
// aligned, bx, by, dsum non-null, 0 <= n_rows <= INT32_MAX, 1 <= n_other <=
// INT32_MAX; a refused call launches nothing.  n_rows == 0 launches nothing.
int launch_lmf_dense(const float* X, const float* bx, int64_t n_rows, int64_t ldx, const float* Y, const float* by,
                     int64_t n_other, int64_t ldy, int64_t f, float* D, int64_t ldd, float* dsum, hipStream_t st);

// The rest of the half-iteration, in place on X, bx, H f32 [n_rows][ldh], hb
// f32 [n_rows], for every row u of the CSR (ptr int64 [n_rows + 1], idx int32 in
// [0, n_other), val f32 > 0), given D and dsum of the OLD tables:
//   s_i = (x . y_i + bx_u) + by_i,  w_i = alpha val_i sig(-s_i)   from the old x
//   g = fma(-reg, x, sum_i w_i y_i - D[u]);  h = fma(g, g, h);  x += lr g / sqrt(1e-6 + h)
//   gb = sum_i w_i - dsum[u];  hb = fma(gb, gb, hb);  bx += lr gb / sqrt(1e-6 + hb)
// in fp32, the item sums in CSR order (a long row: see lmf_long_row).  Row u
// reads row u of X, bx, H, hb, D, dsum and Y, by only, so the bits do not
// depend on the grid.  lr == 0 leaves X and bx bit for bit and still updates
// H, hb.  An id outside [0, n_other) sets *err (device, nullable) and is clamped
// to 0.  Preconditions as launch_lmf_dense for (Y, ldy), (X, ldx), (D, ldd),
// (H, ldh), plus alpha > 0, reg >= 0, lr >= 0, all finite; a refused call
// launches nothing.
int launch_lmf_update(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                      const float* by, int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f,
                      const float* D, int64_t ldd, const float* dsum, float* H, int64_t ldh, float* hb, float alpha,
                      float reg, float lr, int* err, hipStream_t st);

}  // namespace ps
