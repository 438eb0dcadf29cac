// The PinSage head as fused row-block kernels (head.hip): out_dim o a multiple
// of 4, <= 128.
#pragma once
#include "common.h"

namespace ps {

// H1 = lrelu(y G1^T + b1), Z = H1 G2^T over the *nrows (<= max_rows) rows of y
int launch_head_fwd(const float* y, int o, const int* nrows, int64_t max_rows, const float* G1w,
                    const float* G1b, const float* G2w, float* H1, float* Z, hipStream_t st);

// From the loss's accumulators: dZ = sum_c K[c] G[c] (written for dG2; G and Kc
// left zero); dP1 = (dZ G2) * lrelu'(H1); dY = dP1 G1; then the top conv
// layer's normalisation backward, dp = lrelu'(y) * (dY - y (y . dY)) / nrm.
struct HeadBwdParams {
  float* G = nullptr;  // [3][S_max][o]
  int* Kc = nullptr;   // [3][S_max]
  int64_t S_max = 0;
  float* dZ = nullptr;
  int o = 0;
  const int* nrows = nullptr;
  int64_t max_rows = 0;
  const float* H1 = nullptr;
  const float* G1w = nullptr;
  const float* G2w = nullptr;
  const float* y = nullptr;
  const float* nrm = nullptr;
  float* dP1 = nullptr;
  float* dp = nullptr;
  // Gp set (launch_loss without rep_sum): the repeated ranks' per-position
  // rows are summed here, in position order; needs rank_off and pos_sorted
  const int* rank_off = nullptr;
  const int32_t* pos_sorted = nullptr;
  const float* Gp = nullptr;
};
int launch_head_bwd(const HeadBwdParams& p, hipStream_t st);

}  // namespace ps
