// Cosine k-nearest neighbours over an embedding table (knn.hip).
#pragma once
#include "common.h"

namespace ps {

// scratch bytes for batches of qb query rows over n table rows
int64_t knn_scratch_bytes(int64_t n, int64_t qb);

// out_w / out_n [nq][k]: the k largest dot(e_q, e_j) / (|e_q| |e_j| + eps) over
// the n rows of emb (d floats, row stride ld), sorted (sim desc, index asc).
// The query batch is sized to scratch_bytes; a query id outside [0, n) sets *err.
int launch_knn_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries, int64_t nq,
                      int64_t k, float eps, void* scratch, int64_t scratch_bytes, float* out_w, int64_t* out_n,
                      int* err, hipStream_t st);

// largest k of any selection here (kKnnMaxK)
int knn_max_k();

// The same selection over Jaccard scores (cooc.hip's second half): row b of
// counts int32 [m][n] holds the co-occurrence counts of a query of degree
// qdeg[b] with every track, deg int32 [n] the tracks' degrees;
//   s(b, t) = float(co) / (float(qdeg[b] + deg[t] - co) + 1e-10f)   (fp32, IEEE division)
// out_w / out_n [m][k]: the k largest, sorted (s desc, index asc).  counts must
// be 16-byte aligned when n % 4 == 0, and so must deg; m <= 65535.
int launch_knn_select_jaccard(const int32_t* counts, int64_t n, const int32_t* deg, const int32_t* qdeg, int64_t m,
                              int64_t k, float* out_w, int64_t* out_n, hipStream_t st);

// The same selection over finished scores: row b of scores float [m][n] holds
// values >= 0 (no NaN); out_w / out_n [m][k]: the k largest, sorted (score desc,
// index asc), out_w the scores' own bits.  scores must be 16-byte aligned when
// n % 4 == 0; m <= 65535.
int launch_knn_select_score(const float* scores, int64_t n, int64_t m, int64_t k, float* out_w, int64_t* out_n,
                            hipStream_t st);

// scratch bytes for rank batches of qb query rows over n table rows
int64_t rank_scratch_bytes(int64_t n, int64_t qb);
// most targets one query row may own (kRankMaxGroup)
int rank_max_group();

// out_rank [np]: for query row u and each of its targets t = targets[i],
// grp_ptr[u] <= i < grp_ptr[u + 1], the number of rows j that come before t in
// launch_knn_cosine's order for queries[u] (same key function):
//   #{ j : key(j) > key(t) or (key(j) == key(t) and j < t) }.
// grp_ptr is a HOST array [nu + 1] from 0 to np (checked before any launch; a
// group holds at most rank_max_group() targets, a query id may repeat across
// rows); queries, targets and out_rank are device arrays.  An id outside
// [0, n) sets *err (device, nullable) and is clamped.
int launch_rank_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries, int64_t nu,
                       const int64_t* grp_ptr, const int64_t* targets, int64_t np, float eps, void* scratch,
                       int64_t scratch_bytes, int64_t* out_rank, int* err, hipStream_t st);

}  // namespace ps
