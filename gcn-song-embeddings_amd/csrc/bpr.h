// Bayesian personalised ranking (Rendle, Freudenthaler, Gantner, Schmidt-Thieme,
// "BPR: Bayesian Personalized Ranking from Implicit Feedback", 2009) as this
// project defines it: negatives from a counter-based generator and Jacobi
// AdaGrad half-iterations (bpr.hip), so that the model is a function of its
// inputs.  No parity with a package is claimed.
//
// Inputs and tables.  R [n_users, n_items] is a CSR whose rows are strictly
// ascending; only its structure is used, every stored cell is one positive.
// Tables X [n_users, f], Y [n_items, f] and an item bias b [n_items]; there is
// no user bias.  Cell e is the e-th stored cell of R; sample t = e * S + s for
// s < S = negatives.
//
// The draw.  For draw round rho, sample t of a cell (u, i), and tries k = 0 .. 15:
//   (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (rho * 16 + k, t lo, t hi, offset))
//   j = (uint64(r0) * n_items) >> 32
//   accept the first j that is not a column of row u   (binary search; j == i is therefore rejected)
// After 16 rejected tries the sample is void: neg[t] = -1, w[t] = 0.  Otherwise
// neg[t] = j and, with z = (x_u . y_i + b_i) - (x_u . y_j + b_j), w[t] = sig(-z).
// The dot is the row plan's: two columns per lane, fmaf(x.x, y.x, x.y * y.y),
// then the wave sum.  The sigmoid is lmf_sigmoid.  neg and w of sample t depend
// on (seed, rho, offset, t, row u, the tables) only; they do not depend on the
// grid or on batching.
//
// One iteration `it`.  The user half uses draw round 2 it; the item half uses
// round 2 it + 1 and the new X.  Both halves are Jacobi.
//   User half, row u, entries in ascending t, for each t (+w_t, y_i) then
//   (-w_t, y_j).  A void sample contributes (+-0, y_i).
//   Item half, row i: first the samples whose positive is i, in ascending t,
//   with (+w_t, x_u); then the non-void samples whose negative is i, in
//   ascending t, with (-w_t, x_u).
// Each half then runs, in fp32, per row:
//   a = 0;  a = fma(val_e, row_e, a) over the entries in that order;   sv = sum of val_e
//   g = fma(-reg, x, a);  h = fma(g, g, h);  x += lr g / sqrt(1e-6 + h)
//   item half only:  gb = sv;  hb = fma(gb, gb, hb);  b += lr gb / sqrt(1e-6 + hb)      (bias not regularised, as in LMF)
// The accumulators start at zero.  For a fixed draw this is ascent on
// sum_t ln sig(z_t) - (reg/2)(|X|^2 + |Y|^2) over non-void t.
#pragma once
#include "common.h"

namespace ps {

// tries per sample before it is void
int bpr_max_tries();

// neg int32 [nnz S] and w f32 [nnz S] as defined above, for every row of the CSR
// (ptr int64 [n_rows + 1] from 0, idx int32 strictly ascending within a row)
// against X f32 [n_rows][ldx], Y f32 [n_other][ldy] and by f32 [n_other]; no
// table is written.  The call's cell e is cell cell_base + e of R, so that a
// block of rows handed over alone (its ptr rebased to 0, its idx, rows of X and
// outputs) draws what it draws in the whole matrix.  One wave per row of at
// most lmf_long_row() cells, a lane per sample for the draw and the wave for
// the two dots of each sample; a longer row is the workgroup's, wave w taking
// the 64-sample groups w, w + 8, ...  Samples are independent: there is no
// reduction.  A positive id outside [0, n_other) sets *err (device, nullable)
// and is clamped to 0.  Needs 4 <= f <= 128, f % 4 == 0, every ld >= f and
// % 4 == 0, X and Y 16-byte aligned, ptr and by non-null, 0 <= n_rows <=
// INT32_MAX, 1 <= n_other <= INT32_MAX, 1 <= S <= 8, 0 <= rho < 2^27,
// cell_base >= 0; a refused call launches nothing.  n_rows == 0 launches nothing.
int launch_bpr_sample(const int64_t* ptr, const int32_t* idx, int64_t n_rows, int64_t cell_base, const float* X,
                      int64_t ldx, const float* Y, const float* by, int64_t n_other, int64_t ldy, int64_t f, int64_t S,
                      uint64_t seed, int64_t rho, uint32_t offset, int32_t* neg, float* w, int* err, hipStream_t st);

// The signed gathered row sum and the AdaGrad step above, in place on X, H f32
// [n_rows][ldh] and, unless both are null, bx and hb f32 [n_rows], for every row
// of the CSR (ptr int64 [n_rows + 1], idx int32 in [0, n_other), val f32 of
// either sign) against Y f32 [n_other][ldy]:
//   a = fma(val_e, y_e, a) in CSR order from a = 0;  sv = sv + val_e from 0
//   g = fma(-reg, x, a);  h = fma(g, g, h);  x = x + lr * g / sqrt(1e-6 + h)
//   gb = sv;  hb = fma(gb, gb, hb);  bx = bx + lr * gb / sqrt(1e-6 + hb)
// Row forms as launch_lmf_update (a row above lmf_long_row() entries: the
// workgroup, partial sums of a and of sv added in wave order).  lr == 0 leaves
// X and bx bit for bit and still updates H and hb.  A row without entries and
// with reg = 0 has g = 0 and keeps x exactly.  An id outside [0, n_other) sets
// *err (device, nullable) and is clamped to 0.  Preconditions as
// launch_lmf_update for (Y, ldy), (X, ldx), (H, ldh), plus ptr non-null, bx and
// hb both null or both non-null, reg >= 0, lr >= 0, both finite; a refused call
// launches nothing.
int launch_bpr_apply(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                     int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f, float* H, int64_t ldh,
                     float* hb, float reg, float lr, int* err, hipStream_t st);

}  // namespace ps
