// node2vec (Grover & Leskovec 2016) as this project defines it: second-order
// (p, q) walks by rejection sampling on a counter-based generator, and skip-gram
// with negative sampling fitted on the EXPECTED negatives, a closed objective
// over the window co-occurrence counts of the walks (n2v.hip).  No parity with
// a package is claimed.
//
// The walk.  The graph is an undirected CSR: ptr int64 [n_nodes + 1], idx int32
// ascending within a row, no duplicates, no self loops; cum int64 [nnz] holds
// per row the inclusive prefix sum of positive integer edge weights (null:
// unweighted, every weight 1).  Walk k of a call starts at starts[k]; its
// generator position is pos = walk_base + k.  Step j >= 1, try t = 0, 1, ..:
//   (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (j * 256 + t, pos lo, pos hi, offset))
//   total = the current row's last cum (its degree when unweighted)
//   pick  = ((r0 | r1 << 32) * total) >> 64                       (__umul64hi)
//   candidate = the first edge of the row whose cum exceeds pick  (binary search;
//               idx[row start + pick] when unweighted)
//   step 1 takes try 0's candidate.  From step 2 on
//     beta = inv_p  if the candidate is the previous node,
//            1      if it is a neighbour of the previous node (binary search in that row),
//            inv_q  otherwise;            M = max(inv_p, 1, inv_q)
//     accept iff (float)(r2 >> 8) * 0x1p-24f * M < beta
//   (the first product is exact, so this is one fp32 multiply and one compare);
//   after 256 rejected tries the last candidate is taken.
// A proposal is drawn by edge weight and accepted with probability beta / M, so
// the accepted next node has probability proportional to weight * beta.  With
// M / min(beta) <= 16 a try is accepted with probability >= 1/16 and the cap of
// 256 tries distorts at most (15/16)^256 ~ 7e-8 of the steps.  A node without
// edges ends the walk: the remaining positions are -1.
#pragma once
#include "common.h"

namespace ps {

// walks int32 [n_walks][length], walk k in row k, position 0 its start.  One
// lane per walk; a walk reads (seed, offset, walk_base + k, its start, the
// graph) only, so the result does not depend on the grid or on how the walks
// are batched into calls.  A start or neighbour id outside [0, n_nodes) sets
// *err (device, nullable) and is clamped to 0.  Refused with kErrArg, nothing
// launched: inv_p or inv_q not finite or not positive; max(inv_p, 1, inv_q) /
// min(inv_p, 1, inv_q) > 16; length < 1 or >= 2^24; n_nodes < 1 or > INT32_MAX;
// n_walks < 0 or > INT32_MAX; walk_base < 0; a null ptr or idx; a null starts or
// walks unless n_walks == 0, which launches nothing.
int launch_n2v_walk(const int64_t* ptr, const int32_t* idx, const int64_t* cum, int64_t n_nodes,
                    const int64_t* starts, int64_t n_walks, int64_t length, float inv_p, float inv_q, uint64_t seed,
                    uint32_t offset, int64_t walk_base, int32_t* walks, int* err, hipStream_t st);

// Skip-gram with expected negatives.  C [n, n] is the symmetric CSR of window
// co-occurrence counts, #(w) = sum_c C_wc, P(c) proportional to #(c)^0.75,
// tables U (centre), V (context), s_wc = u_w . v_c, no biases.  The objective
// to maximise is
//   L = sum_wc C_wc log sig(s_wc) + K sum_w #(w) sum_c P(c) log sig(-s_wc)
//       - (reg / 2)(|U|^2 + |V|^2)
// and a half-iteration (Jacobi, AdaGrad from zero) runs per row u of X against
// all of Y, with a column weight cw and a row weight rw:
//   D[u] = sum_all i cw_i sig(x_u . y_i) y_i                     (launch_sgns_dense)
//   g    = sum_obs val_i sig(-(x_u . y_i)) y_i - rw_u D[u] - reg x_u
//   h   += g^2;   x_u += lr g / sqrt(1e-6 + h)                   (launch_sgns_update)
// Centre half: X = U, Y = V, cw = P, rw = K #(w).  Context half: X = V, Y = U,
// cw = K #(w), rw = P(c).

// D f32 [n_rows][ldd] (columns [0, f)) for every row of X f32 [n_rows][ldx]
// against all of Y f32 [n_other][ldy], cw f32 [n_other]: the WEIGHT form of
// sig_dense_kernel (sig_dense.h), launch_lmf_dense's kernel with p = cw_i *
// sig(s) in place of sig(s + bx + by) and no row sums.  Exact-f32 MFMA, scores
// in registers only, items in ascending order, no atomics and no
// cross-workgroup sum: the bits of row u depend on x_u, Y and cw only.
// Preconditions and refusals as launch_lmf_dense, with cw non-null.
int launch_sgns_dense(const float* X, int64_t n_rows, int64_t ldx, const float* Y, const float* cw, int64_t n_other,
                      int64_t ldy, int64_t f, float* D, int64_t ldd, hipStream_t st);

// In place on X, H f32 [n_rows][ldh] for every row u of the CSR (ptr int64
// [n_rows + 1], idx int32 in [0, n_other), val f32 > 0), given D of the OLD X,
// in fp32 and in this order, per column:
//   s_i = sum over the wave of fma(x.x, y.x, x.y * y.y)         (two columns per lane)
//   w_i = val_i * sig(-s_i);   a = fma(w_i, y_i, a)             in CSR order from a = 0
//   g   = fma(-reg, x, fma(-rw_u, D[u], a));   h = fma(g, g, h)
//   x   = x + lr * g / sqrt(1e-6 + h)
// Row forms as launch_lmf_update (a row above lmf_long_row() items: the
// workgroup, partial sums added in wave order).  lr == 0 leaves X bit for bit
// and still updates H.  A row without items and with rw_u = 0, reg = 0 has g = 0
// and keeps x exactly: the step is 0 / sqrt(1e-6 + h), never NaN.  An id outside
// [0, n_other) sets *err (device, nullable) and is clamped to 0.  Preconditions
// as launch_lmf_update for (Y, ldy), (X, ldx), (D, ldd), (H, ldh), plus ptr and
// rw non-null, reg >= 0, lr >= 0, both finite; a refused call launches nothing.
int launch_sgns_update(const int64_t* ptr, const int32_t* idx, const float* val, const float* rw, int64_t n_rows,
                       const float* Y, int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* D,
                       int64_t ldd, float* H, int64_t ldh, float reg, float lr, int* err, hipStream_t st);

}  // namespace ps
