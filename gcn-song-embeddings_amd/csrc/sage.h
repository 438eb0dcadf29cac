// Unsupervised GraphSAGE (Hamilton, Ying, Leskovec 2017) as this project
// defines it: the reference's GraphSAGE baseline (baselines.py:517-544 on
// lib/gnns/GNNs_unsupervised.py) cannot run as written, so there are no
// reference numbers; the model is stated here in full and is a function of its
// inputs (counter-based draws, fixed summation orders).  The new integer and
// loss kernels are in sage.hip; the dense work runs on launch_gemm (gemm.h),
// pinsage_segment_wmean (gnns.hip) and launch_adam.
//
// Graph and features.  The graph is an undirected CSR: ptr int64 [n + 1], idx
// int32 ascending within a row, no duplicates, no self loops, weight int64 [nnz]
// positive (null: unweighted).  Features X0 f32 [n, d_in].  Two layers with
// weights W1 [out, 2 d_in] and W2 [out, 2 out], no bias.
//
// Neighbour sample (r, v): round r, fanout S (1 <= S <= 32), node v with row
// length deg.
//   deg <= S: positions 0 .. deg - 1 in CSR order; the other S - deg slots are
//     void (nb = -1, w = 0).
//   otherwise Floyd's algorithm, for j = 0 .. S - 1:
//     m = deg - S + j + 1
//     (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (r * 64 + j, v lo, v hi, offset))
//     t = ((r0 | r1 << 32) * m) >> 64
//     c_j = m - 1 if t is among c_0 .. c_{j-1}, else t
//   slot j holds nb = idx[row start + c_j]; its raw weight is a_j =
//   sqrtf((float)weight_e) (1 when unweighted: the reference mask's sqrt(edge
//   count)); w_j = a_j / (a_0 + a_1 + ...), the sum in slot order from 0 in fp32,
//   then one division (the reference's L1 normalisation).
// The sample depends on (seed, offset, r, v, row v) only.
//
// Positives of step r, batch b_0 .. b_{B-1}: walk w < N_WALKS of anchor i is
// launch_n2v_walk on the same graph with inv_p = inv_q = 1, length WALK_LEN + 1,
// offset 0 and position (r * B_max + i) * N_WALKS + w; positions 1 .. WALK_LEN
// are the P = N_WALKS * WALK_LEN positive slots in walk-major order.  A slot is
// void if it is -1 or equals the anchor.
//
// Negatives: Q slots per anchor a, sample s < Q, tries k = 0 .. 15:
//   ctr = (r * 16 + k, (a Q + s) lo, hi, offset);  j = (uint64(r0) * n) >> 32
//   accept the first j with j != a that is not in row a (binary search); void
//   (-1) after 16 rejections.
// The reference excludes the whole 5-hop ball, which on a projected track graph
// is nearly every node; one hop is used here.
//
// Forward.  Group of anchor i: G = 1 + P + Q slots (anchor, positives,
// negatives).  T = the B G slot nodes with repeats, void slots as node 0 and
// flagged.  Layer 2 uses sample (2r + 1, t) for t in T; U = the sorted unique
// set of T and its neighbours; layer 1 uses sample (2r, u) for u in U.
//   H1[u] = lrelu(W1 [X0[u] || sum_j w_j X0[nb_j]])
//   Z[t]  = lrelu(W2 [H1[t] || sum_j w_j H1[nb_j]])
// lrelu is the GEMM epilogue's leaky ReLU, slope kSlope (the reference: ReLU).
//
// Loss.  c(a, x) = z_a . z_x / max(sqrt(|z_a|^2 |z_x|^2), 1e-8).  Over the
// non-void slots c_pos = the smallest positive cosine, c_neg = the largest
// negative cosine, ties to the lowest slot (the reference's min / max of
// log sig(cos): log sig is monotone).
//   loss_a = max(0, log sig(c_neg) - log sig(c_pos) + margin)
// An anchor is active with at least one non-void positive and one non-void
// negative; loss = sum over active anchors / max(1, #active).  Only the rows a,
// pos*, neg* of a group receive gradient.  Backward and Adam on the existing
// kernels: DESIGN.md has the launch list.
#pragma once
#include "common.h"

namespace ps {

constexpr int kSageMaxFanout = 32;
constexpr int kSageTries = 16;
constexpr int kSageMaxNeg = 16;
constexpr int kSageMaxPos = 64;
constexpr int kSageMaxD = 512;

// nb int32 [m][S], w f32 [m][S]: neighbour sample (round, nodes[i]) in row i.
// One 32-lane half of a wave per node, lane j holding draw j; Floyd's rule is
// resolved in S steps of cross-lane reads.  No LDS, no atomics but the error
// word's.  A node id outside [0, n_nodes), or a neighbour id in idx outside it,
// sets *err (device, nullable) and is clamped to 0.  Refused with kErrArg,
// nothing launched: S outside 1..32; round < 0 or >= 2^25; n_nodes outside
// [1, INT32_MAX]; m < 0 or > INT32_MAX; a null ptr or idx; null nodes, nb or w
// unless m == 0, which launches nothing.
int launch_sage_neighbours(const int64_t* ptr, const int32_t* idx, const int64_t* weight, int64_t n_nodes,
                           const int64_t* nodes, int64_t m, int64_t S, uint64_t seed, int64_t round, uint32_t offset,
                           int32_t* nb, float* w, int* err, hipStream_t st);

// neg int32 [B][Q]: the negatives of round `round` for anchors[i] in row i, one
// lane per sample.  An anchor outside [0, n_nodes) sets *err and is clamped to
// 0.  Refused with kErrArg, nothing launched: Q outside 1..16; round < 0 or
// >= 2^27; n_nodes outside [1, INT32_MAX]; B < 0 or > INT32_MAX; a null ptr or
// idx; null anchors or neg unless B == 0, which launches nothing.
int launch_sage_negatives(const int64_t* ptr, const int32_t* idx, int64_t n_nodes, const int64_t* anchors, int64_t B,
                          int64_t Q, uint64_t seed, int64_t round, uint32_t offset, int32_t* neg, int* err,
                          hipStream_t st);

// The margin loss above and its gradient, one wave per anchor group.  Z f32
// [B G][ldz], G = 1 + P + Q, row a G + g the embedding of slot g of group a;
// slots int32 [B][G], a negative entry marks a void slot (its row of Z is read
// and ignored).  A lane holds columns 2 lane + 128 c, 2 lane + 128 c + 1 of a
// row for c < ceil(d / 128); a dot product or squared norm is the lane's fma
// chain over its columns in ascending order, fmaf(x.x, y.x, x.y * y.y) first,
// then the wave sum.  Selection runs in slot order with strict comparisons.  It
// is lane 0's scalar loop run by every lane: wave_sum is an xor butterfly, at
// each step lanes i and i ^ o add the same two values and fp32 addition is
// commutative, so all 64 lanes hold the same bits of every dot and norm, reach
// the same choice and nothing is broadcast.  The kernel relies on that
// identity: a reduction that leaves the sum in one lane only, or sums in a
// lane-dependent order, would need lane 0's choice handed to the others.
//   loss[a] = loss_a (0 for an inactive anchor), active[a] = 0 / 1,
//   sel[a] = {chosen positive slot, chosen negative slot} (index in the group,
//   -1 without a non-void one),
//   dZ [B G][lddz] = *scale * d loss_a / d Z: all G rows of every group are
//   written, zeros where nothing flows, so no memset is needed before it.
// A pair whose sqrt(|z_a|^2 |z_x|^2) is at most 1e-8 has cosine dot / 1e-8 and
// the gradient of that expression: a zero row gives cosine 0, never NaN.
// Refused with kErrArg, nothing launched: d outside [4, 512] or d % 4 != 0; ldz
// or lddz below d or not a multiple of 4; Z or dZ not 16-byte aligned; P
// outside 1..64; Q outside 1..16; margin not finite; B < 0 or B G > INT32_MAX;
// a null pointer unless B == 0, which launches nothing.
int launch_sage_margin_loss(const float* Z, int64_t ldz, int64_t d, const int32_t* slots, int64_t B, int64_t P,
                            int64_t Q, float margin, const float* scale, float* loss, int32_t* active, int32_t* sel,
                            float* dZ, int64_t lddz, hipStream_t st);

// dp[i][c] = dy[i][c] * lrelu'(y[i][c]) for i < n, c < d (the backward of the
// GEMM epilogue's leaky ReLU from its output: 1 where y > 0, else kSlope); dp
// may be dy.  d % 4 == 0, leading dimensions >= d and multiples of 4, 16-byte
// aligned pointers; n == 0 launches nothing.
int launch_sage_lrelu_backward(const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t n, int64_t d,
                               float* dp, int64_t ldp, hipStream_t st);

}  // namespace ps
