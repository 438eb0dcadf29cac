// Node sets over the track universe [0, n) as bitmaps (frontier.hip): marking,
// and finalisation into per-word prefix counts, sorted members and a device count.
#pragma once
#include "common.h"

namespace ps {

// u64 words of a bitmap over `universe` ids, and the scan blocks (block_sums
// entries) of its multi-block finalisation
int64_t bitset_words(int64_t universe);
int64_t bitset_blocks(int64_t universe);

// mark n int64 ids (host-known count); an id outside [0, limit) sets *err (nullable)
int launch_mark_i64(unsigned long long* bits, const int64_t* ids, int64_t n, int64_t limit, int* err,
                    hipStream_t st);

// mark nb[members[f]][t] for f < *count (<= max_count), t < T (table row stride ld)
int launch_mark_table(unsigned long long* bits, const int32_t* members, const int* count, int64_t max_count,
                      const int32_t* nb, int64_t ld, int T, int64_t universe, hipStream_t st);

// the same from n int64 ids, range-checked against limit (*err as launch_mark_i64)
int launch_mark_table_i64(unsigned long long* bits, const int64_t* ids, int64_t n, const int32_t* nb, int64_t ld,
                          int T, int64_t limit, int* err, hipStream_t st);

// The finalisations a mark launch runs itself (its last block to finish, so
// no separate single-block launch follows it): the marked set N (prefix,
// members, count) and optionally S_lo = N | S_l.  ticket: a zeroed int (the
// frontier's bitmap region, which the step's first kernel zeroes; the last
// block also resets it).
struct MarkFinalize {
  int* ticket = nullptr;
  uint32_t* prefN = nullptr;
  int32_t* memN = nullptr;
  int* cntN = nullptr;
  unsigned long long* dstS = nullptr;  // null: N only
  const unsigned long long* bS = nullptr;
  uint32_t* prefS = nullptr;
  int32_t* memS = nullptr;
  int* cntS = nullptr;
};

// launch_mark_table's arguments (N marked from the table rows of S) plus the
// finalisations of the same launch
struct MarkFinalizeParams {
  unsigned long long* bitsN = nullptr;
  const int32_t* membersS = nullptr;
  const int* countS = nullptr;
  int64_t max_count = 0;
  const int32_t* nb = nullptr;
  int64_t ld = 0;
  int T = 0;
  int64_t universe = 0;
  MarkFinalize fz;
};
// whether launch_mark_finalize can run (single-block finalisation)
bool mark_finalize_fits(int64_t universe);
// mark N from the table rows of S and finalise N (and S_lo = N | S_l when
// fz.dstS is set) in the same launch
int launch_mark_finalize(const MarkFinalizeParams& p, hipStream_t st);

// out[f][t] = rank of nb[nodeset[f]][t] in a finalised set (bits, prefix), f < n
int launch_set_rank_table(const int64_t* nodeset, int64_t n, const int32_t* nb, int64_t ld, int T,
                          const unsigned long long* bits, const uint32_t* prefix, int32_t* out, hipStream_t st);

// Finalise a set: dst = a | b (b nullable), prefix, sorted members, device count.
int launch_set_finalize(unsigned long long* dst, const unsigned long long* a, const unsigned long long* b,
                        int64_t universe, uint32_t* block_sums, uint32_t* prefix, int32_t* members, int* count,
                        hipStream_t st);

// zero the bitmaps region [zero, zero + zero_words), mark ids into bits and
// finalise that set (the top frontier of a step); x_n (nullable): also the id
// range x0 .. x0 + *x_n - 1 (the on-the-fly step's virtual nodes, fly.hip)
int launch_top_set(unsigned long long* zero, int64_t zero_words, unsigned long long* bits, const int64_t* ids,
                   int64_t n, int64_t universe, uint32_t* block_sums, uint32_t* prefix, int32_t* members,
                   int* count, hipStream_t st, int64_t x0 = 0, const int* x_n = nullptr);

}  // namespace ps
