// The GAT aggregator of lib/gnns (GNNs_unsupervised.py:449-465 and 555-567,
// GNN_model.aggregate with gat=True, agg_func 'MEAN') as an edge softmax fused
// with the row gather.  Kernels in gnns.hip; arguments are checked by the C-ABI
// (pinsage_gat_*, include/pinsage_hip.h), the launchers below only launch.
//
// A segment i is a node's whole neighbourhood: entries j in [seg_ptr[i],
// seg_ptr[i+1]) with hrow[j] (a row of h) and c[j] >= 0 (sqrt of the edge
// count); own[i] is the h row of the segment's node; a = [a_l | a_r] f32 [2 d].
//   e_ij = a_l . h[own_i] + a_r . h[hrow_j] = s_l[own_i] + s_r[hrow_j]
//   m_ij = (e_ij > 0 ? e_ij : 0.2 e_ij) c_ij
//   kept: m_ij != 0 and hrow_j in [0, n_h)   (and own_i in [0, n_h))
//   p_ij = exp(m_ij - M_i) / sum_kept exp(m_ik - M_i),  M_i = max_kept m_ik
//   out_i = sum_j p_ij h[hrow_j]
// A segment with nothing kept has p = 0 and a zero row.  The reference's
// unshifted exp / max(sum, 1e-12) is the same number wherever that sum is
// finite and >= 1e-12.
//
// Summation orders (all fixed, no atomics): a per-row dot or a per-segment sum
// is the lane's chain over its strided items in ascending order, then the xor
// butterfly wave_sum; a gathered row sum adds the entries in CSR order.
#pragma once
#include "common.h"

namespace ps {

constexpr float kGatSlope = 0.2f;  // Attention.forward's leaky_relu slope
constexpr int kGatDaRows = 128;    // h rows per block of the da partial sums

// s_l[u] = a_l . h[u], s_r[u] = a_r . h[u] for u = rows[t] (rows null: u = t),
// t < n_rows; one wave per row.  A row id outside [0, n_h) is skipped.
void launch_gat_node_scores(const float* h, int64_t ldh, int64_t n_h, int d, const float* a, const int32_t* rows,
                            int64_t n_rows, float* s_l, float* s_r, hipStream_t st);

// out [n_seg][ldo] and p [nnz] as above; one wave per segment, entries taken in
// chunks of 64 whose (p, row) pairs stay in the lanes' registers and are
// broadcast from there while the lanes cover the columns.
void launch_gat_forward(const float* h, int64_t ldh, int64_t n_h, int d, const int64_t* seg_ptr, const int32_t* hrow,
                        const float* c, const int32_t* own, int64_t n_seg, const float* s_l, const float* s_r,
                        float* out, int64_t ldo, float* p, hipStream_t st);

// Per segment: g_ij = dout_i . h[hrow_j], gbar_i = sum_j p_ij g_ij,
//   de[j] = p_ij (g_ij - gbar_i) c_ij (e_ij > 0 ? 1 : 0.2),  s[i] = sum_j de[j].
void launch_gat_backward_edges(const float* h, int64_t ldh, int64_t n_h, int d, const int64_t* seg_ptr,
                               const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg,
                               const float* s_l, const float* s_r, const float* p, const float* dout, int64_t lddo,
                               float* de, float* s, hipStream_t st);

// Per touched h row u = rows_u[t] (ascending, unique), over the transposed CSR
// (segT [n_rows + 1]; entT[k] the entry, segofT[k] its segment) and the CSR of
// the segments whose own row is u (own_ptr [n_rows + 1], own_seg):
//   cr = sum de[entT],  cl = sum s[own_seg]
//   dh[u] = sum p[entT] dout[segofT] + cr a_r + cl a_l
//   coef[t] = cl, coef[n_rows + t] = cr
// then da = [sum_t cl_t h[u_t] | sum_t cr_t h[u_t]] in two stages: partial
// [ceil(n_rows / kGatDaRows)][2 d] per block of rows in row order, then one
// thread per column adding the blocks in order.
void launch_gat_backward_rows(const float* h, int64_t ldh, int64_t n_h, int d, const float* a, const int32_t* rows_u,
                              int64_t n_rows, const int64_t* segT, const int32_t* entT, const int32_t* segofT,
                              const int64_t* own_ptr, const int32_t* own_seg, const float* p, const float* de,
                              const float* s, int64_t nnz, int64_t n_seg, const float* dout, int64_t lddo, float* dh,
                              int64_t lddh, float* coef, float* partial, float* da, hipStream_t st);

}  // namespace ps
