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

}  // namespace ps
