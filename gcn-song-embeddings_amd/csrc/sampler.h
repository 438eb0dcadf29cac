// Importance sampler launchers (sampler.hip): random walk with restart, visit
// counting, libstdc++-exact top-k over the walk trace.
#pragma once
#include "common.h"

namespace ps {

struct MTChunk;  // mt19937.h

// one workgroup per chunk re-twists and tempers its generator snapshot into
// words_per_chunk raw words of out (total words in all)
int launch_mt_expand(const MTChunk* chunks_dev, int64_t n_chunks, int64_t words_per_chunk, int64_t total,
                     uint32_t* out, hipStream_t st);

// trace [n_src][n_hops]; RNG as launch_walk_runs (ppr_topk.h)
int launch_walk(const int64_t* indptr, const int32_t* indices, const int64_t* sources, int64_t n_src,
                int64_t n_hops, float alpha, const uint32_t* raw, uint64_t seed, uint32_t offset,
                int64_t src_base, int32_t* trace, int* err, hipStream_t st);

// topk(k) of visit_prob from the trace; outputs as launch_heap_topk (ppr_topk.h);
// dense_scratch: the dense rows of graphs with k * 64 > n_all
int launch_visit_topk(const int32_t* trace, const int64_t* sources, int64_t n_src, int64_t n_hops,
                      int64_t n_all, int64_t k, void* dense_scratch, double* out_w, int64_t* out_nb,
                      float* out_wn, int32_t* out_nb32, int64_t T_norm, hipStream_t st);

// dense [n_src][n_all] visit_prob (counts / n_hops, the self column zeroed)
int launch_visit_dense(const int32_t* trace, const int64_t* sources, int64_t n_src, int64_t n_hops,
                       int64_t n_all, double* dense, hipStream_t st);

}  // namespace ps
