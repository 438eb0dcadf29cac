// Index-table preparation of the frontier's layers (conv.hip layer_prep_kernel).
#pragma once
#include "common.h"

namespace ps {

// For f < *nS (rows of the layer's node set S_l, sorted ids):
//   self_src[f]   = row of h_l holding node f (rank in S_{l-1} via P_bits, or the id at l = 0)
//   loc[f*T+t]    = rank of nb[id][t] in N_l (row of the Q output)
//   wloc[f*T+t]   = normalised importance weight
// for u < *nN (rows of N_l): q_src[u] = row of h_l holding that node; for the
// top layer pos_rank[i] = rank of ids[i] in S_l; z (nullable) = the layer
// below's dY rows (*z_rows x z_n), zeroed.
struct LayerPrep {
  const int32_t* S_mem;
  const int* nS;
  const int32_t* N_mem;
  const int* nN;
  const unsigned long long* N_bits;
  const uint32_t* N_pref;
  const unsigned long long* P_bits;
  const uint32_t* P_pref;
  const int32_t* nb;
  const float* wn;
  int64_t ldT;
  int32_t* self_src;
  int32_t* q_src;
  int32_t* loc;
  float* wloc;
  const unsigned long long* S_bits;
  const uint32_t* S_pref;
  const int64_t* ids;
  int64_t n_ids;
  int32_t* pos_rank;
  float* z;
  int z_n;
  const int* z_rows;
};
constexpr int kMaxPrepLayers = 4;
struct LayerPreps {
  LayerPrep L[kMaxPrepLayers];
  int n, T;
};

// every layer's tables in one launch (S_max / N_max: the sets' capacities)
int launch_layer_preps(const LayerPrep* p, const int64_t* S_max, const int64_t* N_max, int n, int T, hipStream_t st);

// In-place row L2 normalisation of y [n][out]; norms[r] = ||y_r|| (nullable).
int launch_l2norm_rows(float* y, int64_t n, int out, float* norms, hipStream_t st);

// The n batch positions grouped by their top-set rank (pos_rank), in position
// order: pos_sorted[rank_off[r] .. rank_off[r + 1]) for every rank r <= *nS.
int launch_pos_csr(const int32_t* pos_rank, int64_t n, const int* nS, int* rank_off, int32_t* pos_sorted,
                   hipStream_t st);

// out[i] = Z[pr[i]] for the n positions (rows of d floats)
int launch_gather_out(const float* Z, int d, const int32_t* pr, int64_t n, float* out, hipStream_t st);

// out[i] (row stride ldo) = h[idx[i]] (row stride ldh, n_h rows of d floats), i < n
int launch_gather_rows(const float* h, int64_t ldh, int64_t n_h, int d, const int64_t* idx, int64_t n,
                       float* out, int64_t ldo, hipStream_t st);

// autograd: the output rows' cotangents go into the loss's accumulators (G slab
// 0, K slab 0); dZ = K * G is formed by the fused head backward (or here, for
// the unfused head: scale = true)
int launch_dz_from_dout(const float* dout, int d, const int32_t* pr, int64_t n, const int* nS,
                        int64_t S_max, float* G, int* Kc, float* dZ, bool scale, const int* rank_off,
                        const int32_t* pos_sorted, float* Gp, hipStream_t st);

// out[M][N] (row stride ld) = the sum of S slabs part[s] (slab stride `stride`
// floats), bias_out[M] (nullable) = the sum of bpart[s][M]; adam (nullable):
// Adam on the slice as it is reduced
int launch_reduce_slabs_2d(const float* part, int S, int64_t stride, int M, int N, float* out,
                           int64_t ld, const float* bpart, float* bias_out, const AdamSlice* adam,
                           hipStream_t st);

// agg[f] = sum_t wloc[f*T+t] * q[loc[f*T+t]] for f < *nS (rows of hid floats)
int launch_agg(const float* q, int hid, const int32_t* loc, const float* wloc, int T,
               const int* nS, int64_t S_max, float* agg, hipStream_t st);

// dp = the backward of y = normalize(lrelu(.)) for nrows (device, <= max_rows)
// rows of n floats; also zeroes z (*z_rows x z_n floats, nullable) and zi
// (zi_n ints, nullable)
int launch_norm_lrelu_bwd(const float* y, const float* nrm, const float* dy, int n,
                          const int* nrows, int64_t max_rows, float* dp, float* z, int z_n,
                          const int* z_rows, int* zi, int64_t zi_n, hipStream_t st);

// The triplet loss over B triples of Z rows (positions 3b + c -> row
// pos_rank[3b + c]) and its cotangents per call c in G[c][S_max][d] with the
// occurrence counts Kc.  G and Kc are zero on entry (init_workspace; then the
// head backward (or dz_combine) and the first backward kernel leave them zero).
struct LossParams {
  const float* Z = nullptr;
  int d = 0;
  const int32_t* pos_rank = nullptr;
  int B = 0;
  float margin = 0.f;
  const float* feats = nullptr;  // nullable: the node-feature monitors' table
  int64_t ld_f = 0;
  int d_in = 0;
  const int64_t* batch = nullptr;  // the positions' ids (with feats)
  float* G = nullptr;
  int* Kc = nullptr;
  int64_t S_max = 0;
  const int* nS = nullptr;
  float* dZ = nullptr;        // combine_dz: dZ = sum_c K[c] G[c]
  float* part = nullptr;      // per-block loss partials (launch_loss_monitor)
  float* colpart = nullptr;   // per-block column sums (the variance monitor)
  float* hinge = nullptr;     // nullable: [B] per-triple hinge argument (parity tests read it)
  bool combine_dz = false;
  // false: the consumer (the fused head backward, head.hip) sums the repeated
  // ranks' Gp rows itself, in the same order
  bool rep_sum = false;
  const int* rank_off = nullptr;  // launch_pos_csr's position CSR
  const int32_t* pos_sorted = nullptr;
  float* Gp = nullptr;            // [3B][d] per-position rows of repeated ranks
};
int launch_loss(const LossParams& p, hipStream_t st);

// scal = {loss, node-feature loss, sum |h_q|^2, variance} from launch_loss's partials
int launch_loss_monitor(const float* part, int nparts, const float* colpart, int d, int B, float* scal,
                        hipStream_t st);

// The on-the-fly step's virtual nodes (fly.hip): virtual node j (rank of
// x0 + j in the top set) gets its real id's summed G row, both with K = 1;
// combine_dz as launch_loss.
int launch_fly_fix(float* G, int* Kc, int64_t S_max, int d, const unsigned long long* bits, const uint32_t* prefix,
                   const int* n_x, const int64_t* xids, int64_t x0, int64_t unit, int64_t x_cap, const int* nS,
                   float* dZ, bool combine_dz, hipStream_t st);

// The step's loss arithmetic on outputs given per position (the micro-batched
// step, pinsage_training._train_batch_micro): Z [3][B][d] (call-major), every
// position its own row (no repeated ranks, so the float atomics of det_put
// each add into a zero: exact).  G [3][3B][d]: position (c, b)'s cotangent at
// G[c][c*B + b].  scal: {loss, 0, sum |h_q|^2, variance} -- the same kernels
// and reduction order as pinsage_engine_loss, so the same bits for the same
// rows.  scratch: triplet_loss_scratch_bytes(B, d).
int64_t triplet_loss_scratch_bytes(int64_t B, int64_t d);
int launch_triplet_loss(const float* Z, int B, int d, float margin, float* G, void* scratch, float* scal,
                        hipStream_t st);

// torch.optim.Adam on n floats; coef as AdamSlice::coef
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, const float* coef,
                double beta1, double beta2, float eps, hipStream_t st);

}  // namespace ps
