// Fused importance sampler launchers (ppr_topk.hip): walks written as sorted
// (id, count) runs [n_src][n_hops], then the libstdc++-exact top-k over them.
#pragma once
#include "common.h"

namespace ps {

// One wave per source.  raw set: the MT19937 words of the walks (3 per hop);
// else Philox keyed by (seed; hop, src_base + source position, offset).  A
// zero-degree node sets err[0].
int launch_walk_runs(const int64_t* indptr, const int32_t* indices, const int64_t* sources, int64_t n_src,
                     int n_hops, float alpha, const uint32_t* raw, uint64_t seed, uint32_t offset,
                     int64_t src_base, uint2* runs, int* n_runs, int* err, hipStream_t st);

// The on-the-fly sampler's walks (fly.hip): sources (int64 or int32, whichever
// is set) are C calls' nodes at c * id_unit + id, sorted by call, the calls'
// segment starts and Philox keys on the device (seg[0..C], seeds[c *
// key_stride]); n_src_cap sources at most, the count in seg[C].
int launch_walk_runs_seg(const int64_t* indptr, const int32_t* indices, const int64_t* sources64,
                         const int32_t* sources32, int64_t n_src_cap, const int* seg, int C, const uint64_t* seeds,
                         int key_stride, int64_t id_unit, int n_hops, float alpha, uint32_t offset, uint2* runs,
                         int* n_runs, int* err, hipStream_t st);

// Top k of every source's visit counts: out_w / out_nb [n_src][k] (f64 weights
// and int64 ids, nullable) and out_wn / out_nb32 [n_src][T_norm] (the first
// T_norm, weights divided by the sum of those T_norm; nullable).  A source
// without runs gives zeros with ids 0..k-1 and 0 / 0 = NaN there, as
// visit_topk_kernel does.  n_src_dev (nullable): n_src is a capacity and the
// count is on the device.  hops (nullable): source s divides by hops[s]
// instead of n_hops.
int launch_heap_topk(const uint2* runs, const int* n_runs, int64_t n_src, int n_hops, int k, double* out_w,
                     int64_t* out_nb, float* out_wn, int32_t* out_nb32, int T_norm, hipStream_t st,
                     const int* n_src_dev = nullptr, const int* hops = nullptr);

// The early-stop walks (sample_neighborhood_topt_early_stop, pinsage_model.py:
// 55-86): a source's walk ends where the stop_np-th node reaches stop_nv visits
// (either < 1: never).  runs / n_runs as launch_walk_runs over the hops taken,
// hops[s] their number (launch_heap_topk's divisor).  A zero-degree node or an
// id >= n_items among the hops taken sets err[0] to err_base + s.  Philox (raw
// null): one wave per source.  MT19937: raw holds 3 n_hops words per source
// from the stream's position on; one wave walks the sources in order (a stopped
// source consumes 3 L - 1 words) and writes the words consumed to *words.
constexpr int kStopMaxHops = 2048;
int launch_walk_runs_stop(const int64_t* indptr, const int32_t* indices, const int64_t* sources, int64_t n_src,
                          int n_hops, float alpha, const uint32_t* raw, uint64_t seed, uint32_t offset,
                          int64_t src_base, int stop_np, int stop_nv, uint32_t n_items, uint2* runs, int* n_runs,
                          int* hops, int64_t* words, int* err, int64_t err_base, hipStream_t st);

}  // namespace ps
