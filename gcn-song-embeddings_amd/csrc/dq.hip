// The transposed neighbour aggregation for gfx950: the backward of agg
// (conv.hip, pinsage_model.py:202) towards the q rows.
//
//   csr_count / scan_* / csr_fill   CSR of the neighbour slots by q row and the
//                                   list of <= 16-pair chunks the dq waves walk
//   csr_sort_*                      every row's pairs in source-row order
//   dq_chunk / dq_combine           d(agg) -> d(q) through the CSR, times lrelu'(q)
//
// dq.h's layout is the one description of the buffers all of them share.
#include "common.h"
#include "dq.h"
#include "bf16split.h"

#include <algorithm>
#include <climits>

namespace ps {

#ifndef PS_DQ_CHUNK
#define PS_DQ_CHUNK 16
#endif
constexpr int kDqChunk = PS_DQ_CHUNK;  // <= 16 (the engine's pair blocks), a multiple of 4
constexpr int kDqSplit = 0x100;  // chunk flag: the row's sum is split over several chunks
__host__ __device__ __forceinline__ int n_chunks(int c) { return (c + kDqChunk - 1) / kDqChunk; }

// ---------------------------------------------------------------- transpose (CSR by q row)
// occurrence (slot e = f T + t) at position pos of row u's range: its
// {source row f, weight} goes to entry (pos - off[u]) % kDqChunk of chunk
// cbase[u] + (pos - off[u]) / kDqChunk, so a dq wave reads its chunk's rows
// and weights with one load
__device__ __forceinline__ void put_occ(int2* __restrict__ occ2, const int* __restrict__ off,
                                        const int* __restrict__ cbase, const float* __restrict__ wloc,
                                        int T, int u, int pos, int64_t e) {
  const int local = pos - off[u];
  occ2[(int64_t)(cbase[u] + local / kDqChunk) * kDqChunk + local % kDqChunk] =
      make_int2((int)(e / T), __float_as_int(wloc[e]));
}

// Popular tracks sit in thousands of neighbour lists, so global per-row
// counters are hot.  Up to kMaxRanges x kLdsRows q rows, the rows are cut into
// ranges of kLdsRows and the work into (range, slice of occurrences) items: a
// block reads the slice, histograms the occurrences that fall in its range in
// LDS and touches each row's global counter ctr[u] once (the slice is read once
// per range, from L2 after the first).  One range: one slice per block; more:
// about two items per workgroup.  Beyond that, lanes of a wave with the same
// row combine into one global atomic.
// The count pass (FILL false) adds the occurrences to ctr = cnt.  The fill pass
// walks the same items over ctr = the rows' cursors: the add reserves the
// item's (or the wave's) positions of a row, and every occurrence is put at
// its own (put_occ).
constexpr int kLdsRows = 40960;  // 160 KiB: a workgroup may take all of a CU's LDS
constexpr int kMaxRanges = 64;
constexpr int kCsrRangeGrid = 256;  // one 160-KiB workgroup per CU
template <bool FILL>
__device__ __forceinline__ void csr_traverse(const int32_t* __restrict__ loc, const float* __restrict__ wloc,
                                             int64_t n, int U, int T, int* __restrict__ ctr,
                                             const int* __restrict__ off, const int* __restrict__ cbase,
                                             int2* __restrict__ occ2, int max_ranges, int* hist) {
  const int R = max(1, (U + kLdsRows - 1) / kLdsRows);
  if (R == 1 || R <= max_ranges) {
    const int64_t S = R == 1 ? gridDim.x : (2 * gridDim.x + R - 1) / R;
    const int64_t slice = (n + S - 1) / S;
    const int64_t items = (int64_t)R * S;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
      const int r = (int)(it % R);
      const int u0 = r * kLdsRows, nu = min(kLdsRows, U - u0);
      const int64_t e0 = (it / R) * slice, e1 = min(n, e0 + slice);
      for (int u = threadIdx.x; u < nu; u += blockDim.x) hist[u] = 0;
      __syncthreads();
      for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int u = loc[e] - u0;
        if ((unsigned)u < (unsigned)nu) atomicAdd(hist + u, 1);
      }
      __syncthreads();
      for (int u = threadIdx.x; u < nu; u += blockDim.x)
        if (hist[u]) {
          const int b = atomicAdd(ctr + u0 + u, hist[u]);
          if (FILL) hist[u] = b;  // the item's base in the row
        }
      __syncthreads();  // (count: the next item zeroes hist)
      if (FILL) {
        for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
          const int u = loc[e] - u0;
          if ((unsigned)u < (unsigned)nu) {
            const int pos = atomicAdd(hist + u, 1);
            put_occ(occ2, off, cbase, wloc, T, u0 + u, pos, e);
          }
        }
        __syncthreads();  // the next item zeroes hist
      }
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63LL; base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = base + lane;
    const int32_t u = e < n ? loc[e] : -1;
    unsigned long long rem = __ballot(e < n);
    int pos = 0;
    while (rem) {
      const int leader = __ffsll((long long)rem) - 1;
      const int32_t v = __shfl(u, leader, 64);
      const unsigned long long m = __ballot(u == v);
      int b = 0;
      if (lane == leader) b = atomicAdd(ctr + v, __popcll(m));
      if (FILL) {
        b = __shfl(b, leader, 64);
        if (u == v) pos = b + __popcll(m & ((1ull << lane) - 1));
      }
      rem &= ~m;
    }
    if (FILL && e < n) put_occ(occ2, off, cbase, wloc, T, u, pos, e);
  }
}

__global__ __launch_bounds__(1024) void csr_count_kernel(const int32_t* __restrict__ loc,
                                                         const int* __restrict__ nS, int T,
                                                         const int* __restrict__ nN,
                                                         int* __restrict__ cnt, int* __restrict__ nsplit,
                                                         int max_ranges) {
  extern __shared__ int hist[];
  if (blockIdx.x == 0 && threadIdx.x == 0) *nsplit = 0;  // the scan appends to it
  csr_traverse<false>(loc, nullptr, (int64_t)(*nS) * T, *nN, T, cnt, nullptr, nullptr, nullptr, max_ranges, hist);
}

// Exclusive scans of cnt[0..*n) into off[0..*n] (off[n] = total) and of the
// per-row chunk counts ceil(cnt/kDqChunk), emitting the chunk list the dq
// kernel walks: chunk = {row u, first occurrence}, at most kDqChunk
// occurrences, never spanning two rows.  cnt is zeroed behind the read (kept
// zero for the next step).  Multi-block form: one block per 1024 rows, each
// block sums its predecessors' totals itself.
constexpr int kScanB = 256, kScanPer = 4, kScanChunk = kScanB * kScanPer;
// rows i0 .. i0+per-1 below n: their slots (c) and their chunks (h)
__device__ __forceinline__ void scan_accumulate(const int* __restrict__ cnt, int64_t i0, int per, int64_t n,
                                                int& c, int& h) {
  c = h = 0;
  for (int q = 0; q < per; ++q)
    if (i0 + q < n) {
      const int v = cnt[i0 + q];
      c += v;
      h += n_chunks(v);
    }
}
__device__ __forceinline__ void wave_scan2(int& a, int& b, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const int ya = __shfl_up(a, o, 64), yb = __shfl_up(b, o, 64);
    if (lane >= o) {
      a += ya;
      b += yb;
    }
  }
}
// adds to (p, pc) the sums of the pairs (c, h) of the block's threads below
// this one: a wave scan plus the earlier waves' totals (ws: LDS, free to write)
template <int W>
__device__ __forceinline__ void block_scan2(int c, int h, int (&ws)[2][W], int& p, int& pc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = c, incc = h;
  wave_scan2(inc, incc, lane);
  if (lane == 63) {
    ws[0][wv] = inc;
    ws[1][wv] = incc;
  }
  __syncthreads();
  p += inc - c;
  pc += incc - h;
  for (int i = 0; i < wv; ++i) {
    p += ws[0][i];
    pc += ws[1][i];
  }
}
// off/cursor/chunks for rows i0 .. i0+per-1 from running totals (p, pc); the
// thread whose range holds index n also writes off[n] and the chunk count
__device__ __forceinline__ void scan_emit(int* __restrict__ cnt, int64_t i0, int per, int64_t n,
                                          int& p, int& pc, int* __restrict__ off,
                                          int* __restrict__ cursor, int* __restrict__ cbase,
                                          int2* __restrict__ chunks,
                                          int* __restrict__ nchunks, int2* __restrict__ split,
                                          int* __restrict__ nsplit) {
  for (int q = 0; q < per; ++q) {
    const int64_t i = i0 + q;
    if (i < n) {
      const int v = cnt[i];
      off[i] = p;
      cursor[i] = p;
      cbase[i] = pc;
      cnt[i] = 0;
      const int nc = n_chunks(v);
      // chunk = {row, occurrences (<= kDqChunk) | kDqSplit if the row spans
      // several chunks}; a split row's chunks are written by csr_fill_kernel's
      // blocks in parallel (one thread here would write thousands for a
      // popular row)
      if (nc == 1) chunks[pc] = make_int2((int)i, v);
      if (nc > 1) split[atomicAdd(nsplit, 1)] = make_int2((int)i, pc);  // order is irrelevant
      p += v;
      pc += nc;
    }
    if (i == n) {
      off[n] = p;
      *nchunks = pc;
    }
  }
}
__global__ __launch_bounds__(kScanB) void scan_block_sums_kernel(const int* __restrict__ cnt,
                                                                 const int* __restrict__ n_dev,
                                                                 int2* __restrict__ bsum) {
  __shared__ int red[2][kScanB / 64];
  int c, h;
  scan_accumulate(cnt, (int64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer, kScanPer, *n_dev, c, h);
  c = wave_sum_i(c);
  h = wave_sum_i(h);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = c;
    red[1][threadIdx.x >> 6] = h;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    bsum[blockIdx.x] = make_int2(red[0][0] + red[0][1] + red[0][2] + red[0][3],
                                 red[1][0] + red[1][1] + red[1][2] + red[1][3]);
}
__global__ __launch_bounds__(kScanB) void scan_apply_kernel(int* __restrict__ cnt,
                                                            const int* __restrict__ n_dev,
                                                            const int2* __restrict__ bsum,
                                                            int* __restrict__ off,
                                                            int* __restrict__ cursor,
                                                            int* __restrict__ cbase,
                                                            int2* __restrict__ chunks,
                                                            int* __restrict__ nchunks,
                                                            int2* __restrict__ split,
                                                            int* __restrict__ nsplit) {
  __shared__ int ws[2][kScanB / 64];
  const int64_t n = *n_dev;
  if ((int64_t)blockIdx.x * kScanChunk > n) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int o = 0, oc = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += kScanB) {
    const int2 b = bsum[i];
    o += b.x;
    oc += b.y;
  }
  o = wave_sum_i(o);
  oc = wave_sum_i(oc);
  if (lane == 0) {
    ws[0][wv] = o;
    ws[1][wv] = oc;
  }
  __syncthreads();
  int p = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
  int pc = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
  int c, h;
  scan_accumulate(cnt, i0, kScanPer, n, c, h);
  block_scan2(c, h, ws, p, pc);
  scan_emit(cnt, i0, kScanPer, n, p, pc, off, cursor, cbase, chunks, nchunks, split, nsplit);
}
// single-block form, U <= 1024 * 64
__global__ __launch_bounds__(1024) void scan_small_kernel(int* __restrict__ cnt,
                                                          const int* __restrict__ n_dev,
                                                          int* __restrict__ off,
                                                          int* __restrict__ cursor,
                                                          int* __restrict__ cbase,
                                                          int2* __restrict__ chunks,
                                                          int* __restrict__ nchunks,
                                                          int2* __restrict__ split,
                                                          int* __restrict__ nsplit) {
  __shared__ int wsum[2][16];
  const int U = *n_dev;
  const int per = (U + 1023) / 1024;
  const int i0 = threadIdx.x * per;
  int c, h, p = 0, pc = 0;
  scan_accumulate(cnt, i0, per, U, c, h);
  block_scan2(c, h, wsum, p, pc);
  scan_emit(cnt, i0, per, U, p, pc, off, cursor, cbase, chunks, nchunks, split, nsplit);
  // no range holds index U when U == 1024 * per: thread 1023 ends on the totals
  if (threadIdx.x == 1023 && U == 1024 * per) {
    off[U] = p;
    *nchunks = pc;
  }
}

__global__ __launch_bounds__(1024) void csr_fill_kernel(const int32_t* __restrict__ loc,
                                                        const float* __restrict__ wloc,
                                                        const int* __restrict__ nS, int T,
                                                        const int* __restrict__ nN,
                                                        int* __restrict__ cursor,
                                                        const int* __restrict__ off,
                                                        const int* __restrict__ cbase,
                                                        int2* __restrict__ occ2, int max_ranges,
                                                        const int2* __restrict__ split,
                                                        const int* __restrict__ nsplit,
                                                        int2* __restrict__ chunks) {
  extern __shared__ int hist[];
  // the chunk descriptors of the rows split over several chunks (the scan's split list)
  const int ns = *nsplit;
  for (int si = blockIdx.x; si < ns; si += gridDim.x) {
    const int2 sp = split[si];
    const int v = off[sp.x + 1] - off[sp.x], nc = n_chunks(v);
    for (int j = threadIdx.x; j < nc; j += blockDim.x)
      chunks[sp.y + j] = make_int2(sp.x, min(kDqChunk, v - j * kDqChunk) | kDqSplit);
  }
  csr_traverse<true>(loc, wloc, (int64_t)(*nS) * T, *nN, T, cursor, off, cbase, occ2, max_ranges, hist);
}

// ---------------------------------------------------------------- canonical CSR order
// The fill claims positions with atomics, so the order of a row's {source row
// f, weight} pairs -- and with it the fp32 summation order of the transposed
// aggregation -- would change from run to run.  Both kernels below sort each
// row's pairs by f (unique within a row: a node's top-T list has distinct
// entries), so the step is bitwise reproducible.  They run on the frontier's
// stream right behind the fill, off the step's critical chain.
//
// Rows of one chunk (<= kDqChunk pairs): one wave per chunk, a bitonic network
// over its 16 lanes (shuffles); empty lanes carry INT_MAX keys.  A row split
// over 2..4 chunks (<= 64 pairs, contiguous from its first chunk) is sorted by
// the wave of its first chunk: every lane holds one pair and its place is the
// number of the row's pairs with a smaller source row.
constexpr int kSortWaveRow = 64;
__global__ __launch_bounds__(256) void csr_sort_chunks_kernel(const int2* __restrict__ chunks,
                                                              const int* __restrict__ nchunks,
                                                              const int* __restrict__ off,
                                                              int2* __restrict__ occ2) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = *nchunks;
  for (int64_t ci = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; ci < nch; ci += nw) {
    const int2 dsc = chunks[ci];
    const int n = dsc.y & 0xff;
    if (dsc.y & kDqSplit) {
      if (ci > 0 && chunks[ci - 1].x == dsc.x) continue;  // (not the row's first chunk)
      const int nr = off[dsc.x + 1] - off[dsc.x];
      if (nr > kSortWaveRow) continue;  // (csr_sort_rows_kernel)
      const int2 v = lane < nr ? occ2[ci * kDqChunk + lane] : make_int2(INT_MAX, 0);
      int r = 0;
      for (int j = 0; j < nr; ++j) r += __shfl(v.x, j, 64) < v.x;
      __builtin_amdgcn_wave_barrier();
      if (lane < nr) occ2[ci * kDqChunk + r] = v;
      continue;
    }
    if (n < 2) continue;
    int2 v = make_int2(INT_MAX, 0);
    if (lane < n) v = occ2[ci * kDqChunk + lane];
#pragma unroll
    for (int k = 2; k <= kDqChunk; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const int ox = __shfl_xor(v.x, j, 64), oy = __shfl_xor(v.y, j, 64);
        const bool lower = (lane & j) == 0, up = (lane & k) == 0;
        // ascending block: the lower lane keeps the smaller key
        const bool take = (lower == up) ? (ox < v.x) : (ox > v.x);
        if (take) v = make_int2(ox, oy);
      }
    if (lane < n) occ2[ci * kDqChunk + lane] = v;
  }
}

// Rows split over several chunks (the scan's split list {u, first chunk}):
// the row's n pairs are contiguous from occ2[cbase * kDqChunk], and their
// source rows f are distinct.  One block per row ranks every pair by a bitmap
// of the f range (windows of kRankBits): a pair's sorted position is the
// count of set bits below its own, read from per-word popcount prefixes, so it
// writes itself to its place in `tmp` (no comparison sort: O(range / 32 + n)
// per row), then the sorted row is copied back.
constexpr int kRankWords = 16384;                   // bitmap words per window (64 KiB)
constexpr int64_t kRankBits = (int64_t)kRankWords * 32;
constexpr int kRankLds = kRankWords * 4 * 2 + 64;   // bitmap + word prefixes + scan scratch
__global__ __launch_bounds__(1024) void csr_sort_rows_kernel(const int2* __restrict__ split,
                                                             const int* __restrict__ nsplit,
                                                             const int* __restrict__ off, int2* __restrict__ occ2,
                                                             int2* __restrict__ tmp) {
  extern __shared__ unsigned rk[];
  unsigned* bits = rk;                            // [kRankWords]
  unsigned* pref = rk + kRankWords;               // [kRankWords] exclusive popcount prefix
  int* red = reinterpret_cast<int*>(pref + kRankWords);  // [16] wave partials
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ns = *nsplit;
  for (int si = blockIdx.x; si < ns; si += gridDim.x) {
    const int2 sp = split[si];
    const int n = off[sp.x + 1] - off[sp.x];
    if (n <= kSortWaveRow) continue;  // (sorted by csr_sort_chunks_kernel)
    int2* row = occ2 + (int64_t)sp.y * kDqChunk;
    int2* out = tmp + (int64_t)sp.y * kDqChunk;
    // f range of the row
    int lo = INT_MAX, hi = -1;
    for (int i = tid; i < n; i += blockDim.x) {
      const int f = row[i].x;
      lo = min(lo, f);
      hi = max(hi, f);
    }
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) red[wv] = lo;
    __syncthreads();
    if (tid == 0) {
      int a = red[0];
      for (int w = 1; w < 16; ++w) a = min(a, red[w]);
      red[0] = a;
    }
    __syncthreads();
    lo = red[0];
    __syncthreads();
    if (lane == 0) red[wv] = hi;
    __syncthreads();
    if (tid == 0) {
      int a = red[0];
      for (int w = 1; w < 16; ++w) a = max(a, red[w]);
      red[0] = a;
    }
    __syncthreads();
    hi = red[0];
    __syncthreads();
    int base = 0;  // pairs placed by earlier windows
    for (int64_t w0 = lo; w0 <= hi; w0 += kRankBits) {
      const int nwords = (int)min((int64_t)kRankWords, (hi - w0) / 32 + 1);
      for (int i = tid; i < nwords; i += blockDim.x) bits[i] = 0u;
      __syncthreads();
      for (int i = tid; i < n; i += blockDim.x) {
        const int64_t b = (int64_t)row[i].x - w0;
        if (b >= 0 && b < (int64_t)nwords * 32) atomicOr(bits + (b >> 5), 1u << (b & 31));
      }
      __syncthreads();
      // exclusive prefix of the words' popcounts: each thread a contiguous run
      const int per = (nwords + (int)blockDim.x - 1) / (int)blockDim.x;
      const int i0 = tid * per;
      int s = 0;
      for (int i = i0; i < min(nwords, i0 + per); ++i) s += __popc(bits[i]);
      int inc = s;
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      if (lane == 63) red[wv] = inc;
      __syncthreads();
      int pre = inc - s;
      for (int w = 0; w < wv; ++w) pre += red[w];
      int total = 0;
      for (int w = 0; w < 16; ++w) total += red[w];
      for (int i = i0; i < min(nwords, i0 + per); ++i) {
        pref[i] = (unsigned)pre;
        pre += __popc(bits[i]);
      }
      __syncthreads();
      for (int i = tid; i < n; i += blockDim.x) {
        const int2 v = row[i];
        const int64_t b = (int64_t)v.x - w0;
        if (b >= 0 && b < (int64_t)nwords * 32) {
          const int wd = (int)(b >> 5);
          const int r = base + (int)pref[wd] + __popc(bits[wd] & ((1u << (b & 31)) - 1u));
          out[r] = v;
        }
      }
      base += total;
      __syncthreads();  // (the next window rewrites bits / pref / red)
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) row[i] = out[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- dq
// dpq[u] = lrelu'(q[u]) * sum over the occurrences (f, t) of u in the slot
// table of w[f][t] * dagg[f]   (the transpose of agg, pinsage_model.py:202).
// One wave per chunk of <= kDqChunk occurrences of ONE row u (chunk list from
// the CSR scan; popular tracks, in thousands of neighbour lists, span many
// chunks).  A chunk is {u, n | split} plus its n {row f, weight} pairs, one
// load each; the wave prefetches its next chunk's pair while it issues this
// chunk's q row and all of its dagg rows at once, so a chunk costs about one
// memory round trip.  A row with one chunk is finished here; a row split over
// several chunks leaves one raw partial per chunk in `part` and
// dq_combine_kernel sums them in chunk order (deterministic, and no
// device-scope float atomics: with per-XCD L2s those run at the memory side
// and serialise on popular rows).
// (A chunk-rows form -- every chunk's masked partial kept as its own row of
// the bottom layer's Q weight gradient GEMM, no combine -- measured even, C2
// 0.451 -> 0.454 ms/step, C4 0.483 -> 0.476, and was removed.)
__device__ __forceinline__ void add4(float4& a, const float4& x) {
  a.x += x.x;
  a.y += x.y;
  a.z += x.z;
  a.w += x.w;
}
// a * lrelu'(q)
__device__ __forceinline__ float4 mask4(const float4& a, const float4& q) {
  return make_float4(a.x * lrelu_grad(q.x), a.y * lrelu_grad(q.y), a.z * lrelu_grad(q.z), a.w * lrelu_grad(q.w));
}

// Row-granular write-through store / L2-bypassing load of one float4 of a
// partial row (the split-row tree below: a partial written on one XCD is read
// by a wave on another, and the XCDs' L2s are not coherent; the same hand-off
// as wgrad.hip's split combine).  `row` must be wave-uniform.
typedef int dq_v4i __attribute__((ext_vector_type(4)));
// dpq row elements e .. e + 3 as their hi / mid / lo bf16 planes (plane stride
// ps elements): the split the long-K weight gradient's fp32 form does in
// registers (bf16split.h), so its planes form (wgrad_pl_kernel) gets the same
// products
__device__ __forceinline__ void dq_store_planes(uint16_t* __restrict__ base, int64_t ps, int64_t e, float4 v) {
  // The planes are the split of the ROUNDED fp32 value.  The tree's root hands
  // in acc * lrelu'(q) straight from the multiply, and the compiler contracted
  // that multiply into the split's first subtraction (v_pk_fma: the residual
  // of the unrounded product), so M and L were not split_planes' of the fp32
  // result where the slope is 0.01.  Opaque registers keep the product rounded.
  float a = v.x, b = v.y, c = v.z, d = v.w;
  asm("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  unsigned h0, m0, l0, h1, m1, l1;
  split_pair(f32x2{a, b}, h0, m0, l0);
  split_pair(f32x2{c, d}, h1, m1, l1);
  *reinterpret_cast<uint2*>(base + e) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(base + ps + e) = make_uint2(m0, m1);
  *reinterpret_cast<uint2*>(base + 2 * ps + e) = make_uint2(l0, l1);
}
__device__ __forceinline__ void dq_st_wt(float* row, int i, float4 v) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, 0x7fffffff, 0x00020000);
  const dq_v4i w{__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), __float_as_int(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(w, rs, (unsigned)i * 16u, 0, 16);
}
__device__ __forceinline__ float4 dq_ld_wt(const float* row, int i) {
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, 0x7fffffff, 0x00020000);
  const dq_v4i y = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)i * 16u, 0, 16);
  return make_float4(__int_as_float(y.x), __int_as_float(y.y), __int_as_float(y.z), __int_as_float(y.w));
}
// Split-row tree (TREE, PINSAGE_DQ_TREE): a row u split over k chunks
// cbase[u] .. cbase[u] + k - 1 is combined by the chunk waves themselves, with
// no dq_combine launch: the chunks are the leaves of a fan-in-8 tree whose node
// (L, g) holds the sum of leaves 8^L g .. 8^L (g + 1) - 1 in part row
// cbase[u] + 8^L g.  A finished node bumps its parent's ticket (level L's
// array, entry cbase[u] + g / 8); the child that arrives last sums the
// parent's children in child order, so every sum has a fixed order whatever
// the timing (deterministic), and the root applies lrelu'(q) and writes
// dpq[u].  Tickets reset themselves.  acc: this chunk's raw partial.
template <int VEC, bool PL3>
__device__ __forceinline__ void dq_tree_leaf(float4 (&acc)[VEC], const float4 (&qv)[VEC], int u, int64_t ci,
                                             int lane, int h4, int hid, const int* __restrict__ off,
                                             const int* __restrict__ cbase, int* __restrict__ tk,
                                             int64_t tk_stride, float* __restrict__ part,
                                             float* __restrict__ dpq, uint16_t* __restrict__ dpq3,
                                             int64_t ps3) {
  const int k = n_chunks(off[u + 1] - off[u]);
  const int64_t cb = cbase[u];
  int64_t g = ci - cb, span = 1, nodes = k;
  float* leaf = part + (int64_t)__builtin_amdgcn_readfirstlane((int)ci) * hid;
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (v * 64 + lane < h4) dq_st_wt(leaf, v * 64 + lane, acc[v]);
  for (int L = 0;; ++L) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this node's row is written through
    const int64_t gp = g >> 3;
    const int nch = (int)min<int64_t>(8, nodes - 8 * gp);
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(tk + L * tk_stride + cb + gp, 1, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    t = __shfl(t, 0, 64);
    if (t != nch - 1) return;  // a sibling still runs: the last one carries on
    if (lane == 0) __hip_atomic_store(tk + L * tk_stride + cb + gp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float4 x[8][VEC];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int cc = c < nch ? c : nch - 1;  // (a repeated child: loaded, not added)
      const float* row = part + (cb + span * (8 * gp + cc)) * hid;
#pragma unroll
      for (int v = 0; v < VEC; ++v) x[c][v] = dq_ld_wt(row, min(v * 64 + lane, h4 - 1));
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = x[0][v];
#pragma unroll
    for (int c = 1; c < 8; ++c)
      if (c < nch)
#pragma unroll
        for (int v = 0; v < VEC; ++v) add4(acc[v], x[c][v]);
    span *= 8;
    nodes = (nodes + 7) >> 3;
    g = gp;
    if (nodes == 1) {  // the root: dpq[u]
      float4* o = reinterpret_cast<float4*>(dpq + (int64_t)u * hid);
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (v * 64 + lane < h4) {
          const float4 r = mask4(acc[v], qv[v]);
          if (PL3) dq_store_planes(dpq3, ps3, (int64_t)u * hid + 4 * (v * 64 + lane), r);
          else o[v * 64 + lane] = r;
        }
      return;
    }
    float* node = part + (int64_t)__builtin_amdgcn_readfirstlane((int)(cb + span * g)) * hid;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (v * 64 + lane < h4) dq_st_wt(node, v * 64 + lane, acc[v]);
  }
}

// Columns c0 .. c0 + 64 VEC - 1 (float4s) of a chunk's q row qr and of its n
// dagg rows (lane j's my_row).  Rows in groups of 4 (n is wave-uniform, so the
// group tests are scalar branches); every load is issued before the first use,
// and a partial group repeats its last row (a cache hit) instead of branching
// per row.
template <int VEC>
__device__ __forceinline__ void dq_load_rows(const float* __restrict__ qr, const float* __restrict__ dagg,
                                             int64_t ld_dagg, int h4, int lane, int c0, int n, int32_t my_row,
                                             float4 (&qv)[VEC], float4 (&x)[kDqChunk][VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) qv[v] = reinterpret_cast<const float4*>(qr)[min(c0 + v * 64 + lane, h4 - 1)];
  const int ng = (n + 3) >> 2;
#pragma unroll
  for (int g = 0; g < kDqChunk / 4; ++g) {
    if (g < ng) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = 4 * g + jj;
        const int32_t row = __shfl(my_row, min(j, n - 1), 64);
        const float4* dr = reinterpret_cast<const float4*>(dagg + (int64_t)row * ld_dagg);
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[j][v] = dr[min(c0 + v * 64 + lane, h4 - 1)];
      }
    }
  }
}
// acc = the chain of the chunk's n fmas w_j x_j, from 0, in pair order
template <int VEC>
__device__ __forceinline__ void dq_fma_rows(int n, float my_w, const float4 (&x)[kDqChunk][VEC],
                                            float4 (&acc)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int ng = (n + 3) >> 2;
#pragma unroll
  for (int g = 0; g < kDqChunk / 4; ++g) {
    if (g < ng) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = 4 * g + jj;
        const float w = j < n ? __shfl(my_w, j, 64) : 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc[v].x = fmaf(w, x[j][v].x, acc[v].x);
          acc[v].y = fmaf(w, x[j][v].y, acc[v].y);
          acc[v].z = fmaf(w, x[j][v].z, acc[v].z);
          acc[v].w = fmaf(w, x[j][v].w, acc[v].w);
        }
      }
    }
  }
}

// PL3 (with TREE; the bottom layer, where only the Q weight gradient reads
// dpq): dpq rows are written as hi / mid / lo bf16 planes (dpq3, plane stride
// ps3) instead of fp32 rows.
template <int VEC, bool TREE, bool PL3>
__global__ __launch_bounds__(256) void dq_chunk_kernel(
    const int2* __restrict__ chunks, const int* __restrict__ nchunks, const int2* __restrict__ occ2,
    const float* __restrict__ dagg, int64_t ld_dagg, const float* __restrict__ q, int hid,
    float* __restrict__ dpq, float* __restrict__ part, const int* __restrict__ off,
    const int* __restrict__ cbase, int* __restrict__ tk, int64_t tk_stride, uint16_t* __restrict__ dpq3,
    int64_t ps3) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int h4 = hid >> 2;
  const int nch = *nchunks;
  int2 dsc = make_int2(0, 0), oc = make_int2(0, 0);
  if (wid < nch) {
    dsc = chunks[wid];
    if (lane < kDqChunk) oc = occ2[wid * kDqChunk + lane];
  }
  if (h4 <= 64 * VEC) {
    // One column pass per chunk: each chunk's result is stored only after the
    // NEXT chunk's rows have been issued.  vmcnt counts stores and loads in
    // issue order, so rows loaded behind a store also waited for it: every
    // chunk paid a store round trip before its loads could land.
    float4 pend[VEC];
    float4* pend_o = nullptr;
    int64_t pend_e = -1;  // (PL3) the pending dpq row's first element
    auto store_pend = [&]() __attribute__((always_inline)) {
      if (PL3 && pend_e >= 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (v * 64 + lane < h4) dq_store_planes(dpq3, ps3, pend_e + 4 * (v * 64 + lane), pend[v]);
        pend_e = -1;
      } else if (pend_o) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (v * 64 + lane < h4) pend_o[v * 64 + lane] = pend[v];
        pend_o = nullptr;
      }
    };
    for (int64_t ci = wid; ci < nch; ci += nw) {
      int2 dsc_n = make_int2(0, 0), oc_n = make_int2(0, 0);
      if (ci + nw < nch) {
        dsc_n = chunks[ci + nw];
        if (lane < kDqChunk) oc_n = occ2[(ci + nw) * kDqChunk + lane];
      }
      const int u = dsc.x, n = dsc.y & 0xff;
      const bool split = (dsc.y & kDqSplit) != 0;
      float4 qv[VEC], x[kDqChunk][VEC], acc[VEC];
      dq_load_rows<VEC>(q + (int64_t)u * hid, dagg, ld_dagg, h4, lane, 0, n, oc.x, qv, x);
      store_pend();  // the previous chunk's result, behind this chunk's loads
      dq_fma_rows<VEC>(n, __int_as_float(oc.y), x, acc);
      if (TREE && split) {  // this chunk is a leaf of its row's tree (no pending store)
        dq_tree_leaf<VEC, PL3>(acc, qv, u, ci, lane, h4, hid, off, cbase, tk, tk_stride, part, dpq, dpq3, ps3);
        dsc = dsc_n;
        oc = oc_n;
        continue;
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) pend[v] = split ? acc[v] : mask4(acc[v], qv[v]);
      if (PL3 && !split) pend_e = (int64_t)u * hid;
      else pend_o = reinterpret_cast<float4*>(split ? part + ci * hid : dpq + (int64_t)u * hid);
      dsc = dsc_n;
      oc = oc_n;
    }
    store_pend();
    return;
  }
  for (int64_t ci = wid; ci < nch; ci += nw) {
    int2 dsc_n = make_int2(0, 0), oc_n = make_int2(0, 0);
    if (ci + nw < nch) {  // the next chunk's descriptor and pairs, under this one
      dsc_n = chunks[ci + nw];
      if (lane < kDqChunk) oc_n = occ2[(ci + nw) * kDqChunk + lane];
    }
    const int u = dsc.x, n = dsc.y & 0xff;
    const bool split = (dsc.y & kDqSplit) != 0;
    float4* o = reinterpret_cast<float4*>(split ? part + ci * hid : dpq + (int64_t)u * hid);
    for (int c0 = 0; c0 < h4; c0 += 64 * VEC) {
      float4 qv[VEC], x[kDqChunk][VEC], acc[VEC];
      dq_load_rows<VEC>(q + (int64_t)u * hid, dagg, ld_dagg, h4, lane, c0, n, oc.x, qv, x);
      dq_fma_rows<VEC>(n, __int_as_float(oc.y), x, acc);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int c = c0 + v * 64 + lane;
        if (c < h4) o[c] = split ? acc[v] : mask4(acc[v], qv[v]);
      }
    }
    dsc = dsc_n;
    oc = oc_n;
  }
}

// dpq[u] = lrelu'(q[u]) * (sum of u's chunk partials) for the rows
// dq_chunk_kernel split (the scan's split list: {u, first chunk}).  One
// 1024-thread block per row: wave w sums partials j = w, w + 16, ... with 8
// loads in flight per lane, then the 16 wave sums are added in a fixed order in
// LDS (deterministic).  Popular rows have hundreds of partials, so a row's sum
// is spread over a block rather than one wave.
constexpr int kCombWaves = 16;
__global__ __launch_bounds__(1024) void dq_combine_kernel(const int2* __restrict__ split,
                                                          const int* __restrict__ nsplit,
                                                          const int* __restrict__ off,
                                                          const float* __restrict__ part,
                                                          const float* __restrict__ q, int hid,
                                                          float* __restrict__ dpq) {
  __shared__ float4 red[kCombWaves][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int h4 = hid >> 2;
  const int ns = *nsplit;
  for (int si = blockIdx.x; si < ns; si += gridDim.x) {
    const int2 sp = split[si];
    const int u = sp.x;
    const int64_t ci = sp.y;
    const int k = (off[u + 1] - off[u] + kDqChunk - 1) / kDqChunk;
    for (int c0 = 0; c0 < h4; c0 += 64) {
      const int c = c0 + lane;
      const int cc = min(c, h4 - 1);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int j = wv;
      for (; j + 7 * kCombWaves < k; j += 8 * kCombWaves) {
        float4 x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          x[i] = reinterpret_cast<const float4*>(part + (ci + j + i * kCombWaves) * hid)[cc];
#pragma unroll
        for (int i = 0; i < 8; ++i) add4(acc, x[i]);
      }
      for (; j < k; j += kCombWaves) add4(acc, reinterpret_cast<const float4*>(part + (ci + j) * hid)[cc]);
      red[wv][lane] = acc;
      __syncthreads();
      if (wv == 0 && c < h4) {
        float4 t = red[0][lane];
        for (int i = 1; i < kCombWaves; ++i) add4(t, red[i][lane]);
        const float4 qq = reinterpret_cast<const float4*>(q + (int64_t)u * hid)[c];
        reinterpret_cast<float4*>(dpq + (int64_t)u * hid)[c] = mask4(t, qq);
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- plan and launchers (dq.h)
// upper bound of the dq chunk list: one partial chunk per row plus full ones
static int64_t dq_chunk_capacity(int64_t S_max, int T, int64_t N_max) {
  return N_max + (S_max * T + kDqChunk - 1) / kDqChunk + 1;
}
// upper bound of the split-row list: a split row holds more than kDqChunk slots
static int64_t dq_split_capacity(int64_t S_max, int T) { return S_max * T / (kDqChunk + 1) + 1; }
// levels of the split-row tree for rows of up to max_chunks chunks (fan-in 8)
static int dq_tree_levels(int64_t max_chunks) {
  int L = 1;
  for (int64_t n = 8; n < max_chunks; n *= 8) ++L;
  return L;
}

DqLayout dq_layout(int64_t S_max, int T, int64_t N_max, int hid) {
  DqLayout a;
  a.S_max = S_max;
  a.N_max = N_max;
  a.T = T;
  a.hid = hid;
  a.max_chunks = dq_chunk_capacity(S_max, T, N_max);
  a.max_split = dq_split_capacity(S_max, T);
  a.tk_len = dq_tree_levels(a.max_chunks) * a.max_chunks;
  int64_t cur = 0;
  auto carve = [&cur](int64_t bytes) {
    const int64_t at = cur;
    cur += align_up(bytes, 256);
    return at;
  };
  a.cnt = carve((N_max + 1) * 4);  // cnt and tk, the zeroed ones, lie together (dq_plan_zero)
  a.tk = carve(a.tk_len * 4);
  a.bsum = carve((int64_t)ceil_div(N_max + 1, kScanChunk) * sizeof(int2) + 16);
  a.off = carve((N_max + 1) * 4);
  a.cursor = carve((N_max + 1) * 4);
  a.cbase = carve((N_max + 1) * 4);
  a.occ2 = carve(a.max_chunks * kDqChunk * sizeof(int2));
  a.occ2_tmp = carve(a.max_chunks * kDqChunk * sizeof(int2));
  a.chunks = carve(a.max_chunks * sizeof(int2));
  a.nchunks = carve(16);
  a.split = carve(a.max_split * sizeof(int2));
  a.nsplit = carve(16);
  a.part = carve(a.max_chunks * hid * 4);
  a.bytes = cur;
  return a;
}

int dq_plan_zero(const DqPlan& p, hipStream_t st) {
  PS_CHECK_HIP(hipMemsetAsync(p.at<char>(p.lay.cnt), 0, (size_t)(p.lay.tk + p.lay.tk_len * 4 - p.lay.cnt), st));
  return kOk;
}

int csr_prepare() {
  static int rc = [] {
    if (hipFuncSetAttribute((const void*)csr_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kLdsRows * 4) != hipSuccess)
      return (int)kErrHip;
    if (hipFuncSetAttribute((const void*)csr_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kLdsRows * 4) != hipSuccess)
      return (int)kErrHip;
    if (hipFuncSetAttribute((const void*)csr_sort_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kRankLds) != hipSuccess)
      return (int)kErrHip;
    return (int)kOk;
  }();
  if (rc != kOk) set_error("csr: cannot raise the dynamic LDS limit");
  return rc;
}

int launch_csr_build(const DqPlan& p, const int32_t* loc, const float* wloc, const int* nS, const int* nN,
                     hipStream_t st) {
  const DqLayout& a = p.lay;
  int* cnt = p.at<int>(a.cnt);
  int* off = p.at<int>(a.off);
  int* cursor = p.at<int>(a.cursor);
  int* cbase = p.at<int>(a.cbase);
  int2* occ2 = p.at<int2>(a.occ2);
  int2* chunks = p.at<int2>(a.chunks);
  int* nchunks = p.at<int>(a.nchunks);
  int2* split = p.at<int2>(a.split);
  int* nsplit = p.at<int>(a.nsplit);
  const int lds = (int)std::min<int64_t>(a.N_max, kLdsRows) * 4;
  // more rows than one histogram: (range, slice) items over a CU-wide grid
  const int gb = a.N_max > kLdsRows ? kCsrRangeGrid : std::max(1, std::min(128, ceil_div(a.S_max * a.T, 2048)));
  // (dq writes every row it owns, no atomics, so dpq needs no zeroing here)
  // PINSAGE_CSR_RANGES: the range cap (0: the per-wave global-atomic path
  // beyond one histogram; A/B and tests)
  const int max_ranges = getenv("PINSAGE_CSR_RANGES") ? atoi(getenv("PINSAGE_CSR_RANGES")) : kMaxRanges;
  hipLaunchKernelGGL(csr_count_kernel, dim3(gb), dim3(1024), lds, st, loc, nS, a.T, nN, cnt, nsplit, max_ranges);
  PS_CHECK_LAUNCH();
  // one block scans small sets; from ~4k rows on its threads' serial runs
  // (N / 1024 rows each) outlast the two-launch form (C4 layer 1, ~15k rows:
  // 26 us in one block)
  if (a.N_max <= 4096) {
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(1024), 0, st, cnt, nN, off, cursor, cbase, chunks, nchunks,
                       split, nsplit);
    PS_CHECK_LAUNCH();
  } else {
    const int nb = ceil_div(a.N_max + 1, kScanChunk);
    int2* bs = p.at<int2>(a.bsum);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nb), dim3(kScanB), 0, st, cnt, nN, bs);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kScanB), 0, st, cnt, nN, bs, off, cursor, cbase, chunks,
                       nchunks, split, nsplit);
    PS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(csr_fill_kernel, dim3(gb), dim3(1024), lds, st, loc, wloc, nS, a.T, nN, cursor, off, cbase, occ2,
                     max_ranges, split, nsplit, chunks);
  PS_CHECK_LAUNCH();
  // canonical pair order (sorted by source row): bitwise-reproducible sums
  hipLaunchKernelGGL(csr_sort_chunks_kernel, dim3(grid_for(a.max_chunks * 64, 256, 2048)), dim3(256), 0, st, chunks,
                     nchunks, off, occ2);
  PS_CHECK_LAUNCH();
  hipLaunchKernelGGL(csr_sort_rows_kernel, dim3(256), dim3(1024), kRankLds, st, split, nsplit, off, occ2,
                     p.at<int2>(a.occ2_tmp));
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_dq_chunks(const DqPlan& p, const float* dagg, int64_t ld_dagg, const float* q, float* dpq,
                     uint16_t* dpq3, int64_t ps3, bool tree, hipStream_t st) {
  const DqLayout& a = p.lay;
  PS_REQUIRE(a.hid % 4 == 0, kErrArg, "dq: hidden dim must be a multiple of 4");
  tree = tree && a.hid <= 512;
  PS_REQUIRE(!dpq3 || tree, kErrArg, "dq: planes output needs the split-row tree and hid <= 512");
  // persistent waves (each prefetches its next chunk); 512 to 4096 blocks
  // measured alike at C2 (round 5), 1024 to 8192 at C2 and C4 (round 6: C4
  // 0.420-0.429 ms/step for all, C2 0.384-0.387), 2048 kept
  const int grid = grid_for(a.max_chunks * 64, 256, 2048);
  // (an XCD-sliced form -- block b on column slice b % 8 of every chunk, so
  // each XCD gathers its eighth of d_agg from its own L2 -- was bitwise this
  // kernel and slower in the step: C2 0.398-0.406 -> 0.408-0.50 ms, C4
  // 0.426-0.431 -> 0.447-0.452, round 6; removed)
  // [2 float4s per lane][combine launch, tree, tree writing planes]
  static constexpr decltype(&dq_chunk_kernel<1, false, false>) kern[2][3] = {
      {dq_chunk_kernel<1, false, false>, dq_chunk_kernel<1, true, false>, dq_chunk_kernel<1, true, true>},
      {dq_chunk_kernel<2, false, false>, dq_chunk_kernel<2, true, false>, dq_chunk_kernel<2, true, true>}};
  hipLaunchKernelGGL(kern[tree ? a.hid > 256 : a.hid >= 512][tree ? (dpq3 ? 2 : 1) : 0], dim3(grid), dim3(256), 0,
                     st, p.at<int2>(a.chunks), p.at<int>(a.nchunks), p.at<int2>(a.occ2), dagg, ld_dagg, q, a.hid,
                     dpq, p.at<float>(a.part), p.at<int>(a.off), p.at<int>(a.cbase), p.at<int>(a.tk), a.max_chunks,
                     dpq3, ps3);
  PS_CHECK_LAUNCH();
  if (tree) return kOk;  // split rows combined by their own chunks (no combine launch)
  hipLaunchKernelGGL(dq_combine_kernel, dim3((int)std::max<int64_t>(1, std::min<int64_t>(a.max_split, 512))),
                     dim3(1024), 0, st, p.at<int2>(a.split), p.at<int>(a.nsplit), p.at<int>(a.off),
                     p.at<float>(a.part), q, a.hid, dpq);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
