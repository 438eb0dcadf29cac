// Beyond-accuracy metrics over recommendation lists (listmetrics.hip).
#pragma once
#include "common.h"

namespace ps {

// inv [n]: 1 / sqrt(sum_c x[r][c]^2) over the n rows of x (d floats, row stride
// ld), IEEE square root and division; a zero row gives +inf.
int launch_row_inv_norms(const float* x, int64_t n, int64_t d, int64_t ld, float* inv, hipStream_t st);

// out [nq]: |sum_{c < kc} inv[id_c] feat[id_c][:]|^2 / kc^2 with id_c =
// lists[i][c] (int64 [nq][ldk], the first kc columns used): the mean of the
// kc x kc cosine matrix of the listed rows, diagonal and repeated ids included.
// A listed zero row (inv = +inf) makes the value NaN.  An id outside [0, n)
// sets *err (device, nullable) and is clamped.
int launch_list_intra_sim(const float* feat, int64_t n, int64_t d, int64_t ld, const float* inv,
                          const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, float* out, int* err,
                          hipStream_t st);

// most list columns launch_list_pair_overlap compares (kOvMaxK)
int list_overlap_max_k();

// out [np][3] int32: |set(A)|, |set(B)|, |set(A) & set(B)| for A = lists[a][:kc],
// B = lists[b][:kc], (a, b) = pairs[p] (int64 [np][2], device).  A row outside
// [0, nq) or an id outside [0, n_ids) sets *err (device, nullable) and is clamped.
int launch_list_pair_overlap(const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, int64_t n_ids,
                             const int64_t* pairs, int64_t np, int32_t* out, int* err, hipStream_t st);

}  // namespace ps
