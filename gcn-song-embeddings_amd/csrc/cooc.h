// Co-occurrence counts of tracks over shared collections, and the Jaccard
// neighbours that stand on them (cooc.hip).
#pragma once
#include "common.h"

namespace ps {

// counters of one LDS tile of the track range (kCoocTile)
int cooc_tile();

// scratch bytes of launch_cooc_jaccard for batches of qb query rows over n_tracks tracks
int64_t cooc_scratch_bytes(int64_t n_tracks, int64_t qb);

// The membership relation as two CSRs without duplicates (device arrays):
// track -> collections t2c_ptr int64 [n_tracks + 1] / t2c_idx int32 (ids in
// [0, n_cols)), collection -> tracks c2t_ptr int64 [n_cols + 1] / c2t_idx int32
// (ids in [0, n_tracks), ascending within a row).
//
// out int32 [nq][n_tracks]: out[i][t] = the number of collections that hold
// both queries[i] and t (baselines.py:211 intersect_sizes[nodeset, :].toarray()).
// Every element is written exactly once; the counts are integer adds, so two
// runs give the same bits.  A query id outside [0, n_tracks) sets *err (device,
// nullable) and is clamped to 0.
int launch_cooc_counts(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                       const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* queries, int64_t nq,
                       int32_t* out, int* err, hipStream_t st);

// out_w / out_n [nq][k]: the k largest Jaccard scores of each query against all
// tracks (launch_knn_select_jaccard's formula, deg[t] = t2c_ptr[t + 1] -
// t2c_ptr[t]), sorted (score desc, index asc): JaccardFast.knn
// (baselines.py:210-220) before it drops column 0.  The queries are batched to
// scratch_bytes as launch_knn_cosine batches them.  Needs 1 <= k <=
// min(n_tracks, 4096) and n_tracks <= INT32_MAX; a refused call launches nothing.
int launch_cooc_jaccard(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                        const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* queries,
                        int64_t nq, int64_t k, void* scratch, int64_t scratch_bytes, float* out_w, int64_t* out_n,
                        int* err, hipStream_t st);

// The weighted form: the same two CSRs read as node -> middle nodes and middle
// node -> nodes (for a graph's own adjacency both are that adjacency), and
// wt int64 [n_cols], a weight per middle node (null only where n_cols == 0):
//   S(q, t) = sum of wt[c] over the middle nodes c that neighbour both q and t,
// in 64-bit integer adds (wrapping), so two runs give the same bits.

// 64-bit counters of one LDS tile of the weighted kernel (kCoocWTile)
int cooc_weighted_tile();

// scratch bytes of launch_cooc_weighted_knn for batches of qb query rows
int64_t cooc_weighted_scratch_bytes(int64_t n_tracks, int64_t qb);

// out int64 [nq][n_tracks]: out[i][t] = S(queries[i], t), every element written
// exactly once; query ids as in launch_cooc_counts.
int launch_cooc_weighted_sums(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                              const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* wt,
                              const int64_t* queries, int64_t nq, int64_t* out, int* err, hipStream_t st);

// out_w / out_n [nq][k]: the k largest of float32(S) * 2^-30 (the int64 ->
// float32 conversion rounds to nearest even) per query, sorted (score desc,
// index asc), by launch_knn_select_score.  Arguments, batching and limits as
// launch_cooc_jaccard; sums must be >= 0.
int launch_cooc_weighted_knn(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                             const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* wt,
                             const int64_t* queries, int64_t nq, int64_t k, void* scratch, int64_t scratch_bytes,
                             float* out_w, int64_t* out_n, int* err, hipStream_t st);

}  // namespace ps
