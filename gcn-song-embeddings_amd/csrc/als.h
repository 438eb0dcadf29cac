// Implicit-feedback ALS: the Gram matrix and one conjugate-gradient
// half-iteration (als.hip).
#pragma once
#include "common.h"

namespace ps {

// rows of one block of rows (= waves of a workgroup): row r is in block r / this
int als_rows_per_block();
// a row with more items than this is solved by a whole workgroup, its item sums
// split over the waves and added in wave order; at most this many: one wave
int als_long_row();

// G f32 [f][f] = Y^T Y + reg I for Y f32 [n][ld] (device).  Fixed summation
// order (every 16th row per partial sum, rows ascending, the 16 partial sums in
// order), no atomics: the same bits on every run, and G is symmetric bit for
// bit.  Needs 4 <= f <= 128, f % 4 == 0, ld >= f, ld % 4 == 0, Y and G 16-byte
// aligned, reg > 0, 0 <= n <= INT32_MAX; a refused call launches nothing.
int launch_als_gram(const float* Y, int64_t n, int64_t f, int64_t ld, float reg, float* G, hipStream_t st);

// One half-iteration: for every row u of the CSR (ptr int64 [n_rows + 1], idx
// int32 in [0, n_other), val f32 > 0), with c = alpha val, x = X[u], y_i = Y[i]:
//   r = -G x + sum_i (c - (c - 1)(y_i . x)) y_i;  p = r;  rs = r . r
//   if rs < 1e-20: X[u] stays;  else cg_steps times:
//     Ap = G p + sum_i (c - 1)(y_i . p) y_i
//     a = rs / (p . Ap);  x += a p;  r -= a Ap;  rn = r . r
//     if rn < 1e-20: break;   p = r + (rn / rs) p;  rs = rn
//   X[u] = x
// in fp32, the item sums in CSR order (a long row: see als_long_row).  G is read
// as (G v)[c] = sum_k G[k][c] v[k] (launch_als_gram's G is symmetric).  Only
// columns [0, f) of X are written; row u reads X[u] and Y only, so the update is
// in place and the bits do not depend on the grid.  cg_steps == 0 launches
// nothing.  An id outside [0, n_other) sets *err (device, nullable) and is
// clamped to 0.  Preconditions as launch_als_gram for (Y, ldy) and (X, ldx),
// plus G 16-byte aligned, alpha > 0 finite, cg_steps >= 0, n_rows and n_other
// <= INT32_MAX, n_other >= 1; a refused call launches nothing.
int launch_als_half(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                    int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* G, float alpha,
                    int64_t cg_steps, int* err, hipStream_t st);

}  // namespace ps
