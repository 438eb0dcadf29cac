// The transposed aggregation (dq.hip): the CSR of the neighbour slots by q row
// with its chunk list, and dpq[u] = lrelu'(q[u]) * the weighted sum of the dagg
// rows whose slots name q row u.
#pragma once
#include "common.h"

namespace ps {

// The plan's buffers as byte offsets from a 256-byte-aligned base.  dq_layout
// is the only place that knows them, their sizes and the capacities.
struct DqLayout {
  int64_t S_max = 0, N_max = 0;  // capacities: source rows (of T slots each), q rows
  int T = 0, hid = 0;
  int64_t max_chunks = 0;  // the chunk list: one partial chunk per q row plus the full ones
  int64_t max_split = 0;   // q rows of more than one chunk
  int64_t tk_len = 0;      // tickets of the split-row tree: its levels x max_chunks
  int64_t cnt = 0;         // int [N + 1] slots per q row
  int64_t tk = 0;          // int [tk_len]
  int64_t bsum = 0;        // block sums of the two-launch scan
  int64_t off = 0;         // int [N + 1] row starts
  int64_t cursor = 0;      // int [N + 1] fill cursors
  int64_t cbase = 0;       // int [N + 1] first chunk of every row
  int64_t occ2 = 0;        // int2 [max_chunks][16] {source row, weight bits} pairs by q row
  int64_t occ2_tmp = 0;    // the same size: the canonical sort's scratch
  int64_t chunks = 0;      // int2 [max_chunks] {q row, pairs | split flag}
  int64_t nchunks = 0;     // int
  int64_t split = 0;       // int2 [max_split] {q row, first chunk}
  int64_t nsplit = 0;      // int
  int64_t part = 0;        // float [max_chunks][hid] partials of the split rows
  int64_t bytes = 0;       // all of it, a multiple of 256
};
DqLayout dq_layout(int64_t S_max, int T, int64_t N_max, int hid);

// the layout over memory: all that the launchers take
struct DqPlan {
  DqLayout lay;
  void* base = nullptr;
  template <class P>
  P* at(int64_t o) const {
    return reinterpret_cast<P*>(static_cast<char*>(base) + o);
  }
};

// cnt and the tickets are zero on entry to every launch below and left zero by
// it (the scan zeroes cnt behind its read, the tickets reset themselves): zero
// them once per plan, here
int dq_plan_zero(const DqPlan& p, hipStream_t st);

// dynamic LDS above 64 KiB must be allowed per kernel (once, outside capture)
int csr_prepare();

// CSR of the neighbour slots by q row, every row's pairs sorted by source row
// (bitwise-reproducible sums), plus the dq chunk list.  loc / wloc [S][T]: the
// q row and the weight of every slot (LayerPrep's); nS / nN: device row counts
// of the source rows and the q rows, at most the plan's capacities.
int launch_csr_build(const DqPlan& p, const int32_t* loc, const float* wloc, const int* nS, const int* nN,
                     hipStream_t st);

// The aggregation's transpose over launch_csr_build's plan, rows of the plan's
// hid floats (dagg's row stride ld_dagg).  tree (taken at hid <= 512): split
// rows are combined by their own chunks, no combine launch; with it dpq3 (plane
// stride ps3, nullable): dpq written as hi / mid / lo bf16 planes instead.
int launch_dq_chunks(const DqPlan& p, const float* dagg, int64_t ld_dagg, const float* q, float* dpq,
                     uint16_t* dpq3, int64_t ps3, bool tree, hipStream_t st);

}  // namespace ps
