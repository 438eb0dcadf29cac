// Co-occurrence counts of tracks over shared collections, and Jaccard nearest
// neighbours on them: the GPU form of JaccardFast (baselines.py:194-220), whose
// train() forms the n_tracks x n_tracks product ctmat^T * ctmat in scipy and
// whose knn() densifies nq rows of it on the host.
//
// Nothing n x n exists here.  The membership relation is held as two CSRs
// (track -> collections, collection -> sorted tracks); the row of the product
// for query q is  co[q][t] = #{ c : q in c and t in c }  =  the sum over q's
// collections of their member lists, and it is produced per batch of queries.
//
// cooc_tile_kernel: grid (track tile, query).  A workgroup owns the counters
// of P::kTile consecutive tracks in LDS: it zeroes them, then for each
// collection of q (one lane per collection) binary-searches the slice of the
// sorted member list that falls into the tile and adds the collection's weight
// per member with LDS atomics, and after a barrier writes the tile to the global
// row with 16-byte stores.  No global atomic, no memset: every element of the
// row is written exactly once, and integer adds make the result independent of
// the order.
//
// The kernel is a template over what a tile accumulates and how it leaves
// (CoocCount / CoocSum / CoocScore below): the counts with weight 1 in int32
// counters, and the weighted two-hop sums of the link-prediction indices
// (Adamic-Adar: SimpleSimilarity, baselines.py:153-191) with an int64 weight
// per middle node in 64-bit counters, half as many to the tile.
//
// The scores and the top k come from knn.hip's selection kernel: under its
// Jaccard key policy straight from the int32 count rows and the degrees, under
// its score policy from the float image of the weighted sums.
#include <algorithm>
#include <type_traits>

#include "cooc.h"
#include "knn.h"

namespace ps {

constexpr int kCoocTileBytes = 64 * 1024;  // counters of one tile: two workgroups per CU
constexpr int kCoocBlock = 512;            // 8 waves, 64 collections each at a time
constexpr int kCoocWide = 32;              // a slice of a member list above this is added by the whole wave
constexpr int kCoocShift = 30;             // fixed point of the weighted sums (baselines.LINKSIM_SHIFT)

// counts: every collection weighs 1; int32 counters, int32 rows
struct CoocCount {
  using Acc = int32_t;
  using Out = int32_t;
  static constexpr bool kWeighted = false;
  static __device__ __forceinline__ Out out(Acc a) { return a; }
};
// weighted sums: int64 weights, 64-bit counters (wrapping adds), int64 rows
struct CoocSum {
  using Acc = unsigned long long;
  using Out = int64_t;
  static constexpr bool kWeighted = true;
  static __device__ __forceinline__ Out out(Acc a) { return (int64_t)a; }
};
// the same sums, leaving as float32(S) * 2^-kCoocShift: the conversion rounds
// to nearest even, the scaling is exact
struct CoocScore {
  using Acc = unsigned long long;
  using Out = float;
  static constexpr bool kWeighted = true;
  static __device__ __forceinline__ Out out(Acc a) {
    return __ll2float_rn((long long)a) * (1.0f / (float)(1 << kCoocShift));
  }
};
template <class P>
constexpr int kCoocTileOf = kCoocTileBytes / (int)sizeof(typename P::Acc);
constexpr int kCoocTile = kCoocTileOf<CoocCount>;    // 16384 int32 counters
constexpr int kCoocWTile = kCoocTileOf<CoocSum>;     // 8192 64-bit counters

// first i in [lo, hi) with a[i] >= v, or hi (a ascending)
__device__ __forceinline__ int64_t cooc_lower_bound(const int32_t* __restrict__ a, int64_t lo, int64_t hi,
                                                    int32_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] >= v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ void cooc_degree_kernel(const int64_t* __restrict__ t2c_ptr, int64_t n, int32_t* __restrict__ deg) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    deg[t] = (int32_t)(t2c_ptr[t + 1] - t2c_ptr[t]);
}

// wt int64 [n_cols]: read by the weighted policies only (null for the counts)
template <class P>
__global__ __launch_bounds__(kCoocBlock) void cooc_tile_kernel(
    const int64_t* __restrict__ t2c_ptr, const int32_t* __restrict__ t2c_idx, const int64_t* __restrict__ c2t_ptr,
    const int32_t* __restrict__ c2t_idx, int64_t n, int64_t n_cols, const int64_t* __restrict__ wt,
    const int64_t* __restrict__ queries, typename P::Out* __restrict__ out, int32_t* __restrict__ qdeg,
    int* __restrict__ err) {
  using Acc = typename P::Acc;
  using Out = typename P::Out;
  constexpr int kTile = kCoocTileOf<P>;
  constexpr int kVec = 16 / (int)sizeof(Out);  // elements of one 16-byte store
  __shared__ __attribute__((aligned(16))) Acc tile[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.y;
  int64_t q = queries[b];
  if (q < 0 || q >= n) {  // callers validate; clamp so that no access strays
    if (err && tid == 0) atomicExch(err, 1);
    q = 0;
  }
  const int64_t lo = (int64_t)blockIdx.x * kTile;           // the tile is tracks [lo, lo + len)
  const int len = (int)min<int64_t>(kTile, n - lo);         // >= 1: the grid has ceil(n / tile) tiles
  for (int i = tid; i < kCoocTileBytes / 16; i += kCoocBlock) reinterpret_cast<int4*>(tile)[i] = make_int4(0, 0, 0, 0);
  __syncthreads();

  const int64_t c0 = t2c_ptr[q], c1 = t2c_ptr[q + 1];
  if (qdeg && blockIdx.x == 0 && tid == 0) qdeg[b] = (int32_t)(c1 - c0);
  auto add = [&](int64_t j, Acc w) __attribute__((always_inline)) {
    const uint32_t o = (uint32_t)(c2t_idx[j] - (int32_t)lo);
    if (o < (uint32_t)len) atomicAdd(&tile[o], w);  // a row out of order cannot leave the tile
  };
  // A lane per collection: the two binary searches are chains of dependent
  // loads, and 64 of them in flight per wave hide what one per wave would not.
  // A lane adds a short slice itself; the wave takes the long ones (a hub
  // collection) together, one at a time.
  for (int64_t base = c0 + (int64_t)wv * 64; base < c1; base += kCoocBlock) {  // wave-uniform
    const int64_t ci = base + lane;
    long long s0 = 0, s1 = 0;
    Acc w = 1;
    if (ci < c1) {
      const int64_t c = t2c_idx[ci];
      if (c >= 0 && c < n_cols) {
        const int64_t r0 = c2t_ptr[c], r1 = c2t_ptr[c + 1];
        // n <= INT32_MAX (the launcher refuses more), so lo + len fits an int32
        s0 = cooc_lower_bound(c2t_idx, r0, r1, (int32_t)lo);
        s1 = cooc_lower_bound(c2t_idx, s0, r1, (int32_t)(lo + len));
        if constexpr (P::kWeighted) w = (Acc)wt[c];
      }
    }
    const bool wide = s1 - s0 > kCoocWide;
    if (!wide)
      for (long long j = s0; j < s1; ++j) add(j, w);
    for (unsigned long long m = __ballot(wide); m; m &= m - 1) {
      const int l = __ffsll((long long)m) - 1;
      const long long a0 = __shfl(s0, l, 64), a1 = __shfl(s1, l, 64);
      Acc wl = 1;
      if constexpr (P::kWeighted) wl = __shfl(w, l, 64);
      for (long long j = a0 + lane; j < a1; j += 64) add(j, wl);
    }
  }
  __syncthreads();

  // 16-byte stores from the first aligned element on; scalar before it and at the tail
  Out* dst = out + b * n + lo;
  const int head = min(len, (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / sizeof(Out)));
  const int nv = (len - head) / kVec;
  if (tid < head) dst[tid] = P::out(tile[tid]);
  if constexpr (std::is_same<Acc, Out>::value) {
    if (head == 0) {
      for (int i = tid; i < nv; i += kCoocBlock)
        reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(tile)[i];
    } else {
      for (int i = tid; i < nv; i += kCoocBlock) {
        const int o = head + 4 * i;
        *reinterpret_cast<int4*>(dst + o) = make_int4(tile[o], tile[o + 1], tile[o + 2], tile[o + 3]);
      }
    }
  } else {
    for (int i = tid; i < nv; i += kCoocBlock) {
      const int o = head + kVec * i;
      union {
        int4 v;
        Out e[kVec];
      } u;
#pragma unroll
      for (int c = 0; c < kVec; ++c) u.e[c] = P::out(tile[o + c]);
      *reinterpret_cast<int4*>(dst + o) = u.v;
    }
  }
  for (int i = head + kVec * nv + tid; i < len; i += kCoocBlock) dst[i] = P::out(tile[i]);
}

int cooc_tile() { return kCoocTile; }

int64_t cooc_scratch_bytes(int64_t n, int64_t qb) {
  return align_up(n * 4, 256) + align_up(qb * 4, 256) + align_up(qb * n * 4, 256) + 256;
}

// the index arrays may be null where the relation is empty (they are never read then)
static int cooc_check(const int64_t* t2c_ptr, const int64_t* c2t_ptr, int64_t n, int64_t n_cols,
                      const int64_t* queries, int64_t nq) {
  PS_REQUIRE(n > 0 && n_cols >= 0 && nq >= 0, kErrArg, "cooc: bad sizes");
  PS_REQUIRE(n <= INT32_MAX && n_cols <= INT32_MAX, kErrArg, "cooc: ids do not fit 32 bits");
  PS_REQUIRE(t2c_ptr != nullptr && c2t_ptr != nullptr, kErrArg, "cooc: null row pointers");
  PS_REQUIRE(queries != nullptr || nq == 0, kErrArg, "cooc: null queries");
  return kOk;
}

// the rows of m <= 65535 queries under policy P into out (rows n apart)
template <class P>
static int cooc_launch_tiles(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                             const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* wt,
                             const int64_t* queries, int64_t m, typename P::Out* out, int32_t* qdeg, int* err,
                             hipStream_t st) {
  hipLaunchKernelGGL(cooc_tile_kernel<P>, dim3((unsigned)ceil_div(n, kCoocTileOf<P>), (unsigned)m), dim3(kCoocBlock),
                     0, st, t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, wt, queries, out, qdeg, err);
  PS_CHECK_LAUNCH();
  return kOk;
}

static int cooc_launch_counts(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                              const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* queries, int64_t m,
                              int32_t* out, int32_t* qdeg, int* err, hipStream_t st) {
  return cooc_launch_tiles<CoocCount>(t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, nullptr, queries, m, out, qdeg,
                                      err, st);
}

int launch_cooc_counts(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                       const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* queries, int64_t nq,
                       int32_t* out, int* err, hipStream_t st) {
  PS_TRY(cooc_check(t2c_ptr, c2t_ptr, n, n_cols, queries, nq));
  PS_REQUIRE(out != nullptr || nq == 0, kErrArg, "cooc: null output");
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
    const int64_t m = std::min<int64_t>(65535, nq - q0);
    PS_TRY(cooc_launch_counts(t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, queries + q0, m, out + q0 * n, nullptr,
                              err, st));
  }
  return kOk;
}

int launch_cooc_jaccard(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                        const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* queries, int64_t nq,
                        int64_t k, void* scratch, int64_t scratch_bytes, float* out_w, int64_t* out_n, int* err,
                        hipStream_t st) {
  PS_TRY(cooc_check(t2c_ptr, c2t_ptr, n, n_cols, queries, nq));
  PS_REQUIRE(k >= 1 && k <= n && k <= knn_max_k(), kErrArg, "cooc: need 1 <= k <= min(n_tracks, 4096)");
  PS_REQUIRE((out_w != nullptr && out_n != nullptr) || nq == 0, kErrArg, "cooc: null output");
  if (nq == 0) return kOk;
  PS_REQUIRE(scratch != nullptr && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0, kErrArg,
             "cooc: scratch must be 16-byte aligned");
  // batch of query rows that fits the scratch
  // (a row costs at least n * 4 bytes: start one above that bound and step down)
  int64_t qb = std::min<int64_t>(nq, 65535);
  qb = std::min<int64_t>(qb, std::max<int64_t>(1, (scratch_bytes - align_up(n * 4, 256)) / (n * 4) + 1));
  while (qb > 1 && cooc_scratch_bytes(n, qb) > scratch_bytes) --qb;
  PS_REQUIRE(cooc_scratch_bytes(n, qb) <= scratch_bytes, kErrWorkspace, "cooc: scratch too small");
  char* s = (char*)scratch;
  int32_t* deg = (int32_t*)s;
  s += align_up(n * 4, 256);
  int32_t* qdeg = (int32_t*)s;
  s += align_up(qb * 4, 256);
  int32_t* counts = (int32_t*)s;

  hipLaunchKernelGGL(cooc_degree_kernel, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, t2c_ptr, n, deg);
  PS_CHECK_LAUNCH();
  for (int64_t q0 = 0; q0 < nq; q0 += qb) {
    const int64_t m = std::min(qb, nq - q0);
    PS_TRY(cooc_launch_counts(t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, queries + q0, m, counts, qdeg, err, st));
    PS_TRY(launch_knn_select_jaccard(counts, n, deg, qdeg, m, k, out_w + q0 * k, out_n + q0 * k, st));
  }
  return kOk;
}

// ---------------------------------------------------------------- weighted sums
int cooc_weighted_tile() { return kCoocWTile; }

int64_t cooc_weighted_scratch_bytes(int64_t n, int64_t qb) { return align_up(qb * n * 4, 256) + 256; }

int launch_cooc_weighted_sums(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                              const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* wt,
                              const int64_t* queries, int64_t nq, int64_t* out, int* err, hipStream_t st) {
  PS_TRY(cooc_check(t2c_ptr, c2t_ptr, n, n_cols, queries, nq));
  PS_REQUIRE(wt != nullptr || n_cols == 0, kErrArg, "cooc: null weights");
  PS_REQUIRE(out != nullptr || nq == 0, kErrArg, "cooc: null output");
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
    const int64_t m = std::min<int64_t>(65535, nq - q0);
    PS_TRY(cooc_launch_tiles<CoocSum>(t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, wt, queries + q0, m,
                                      out + q0 * n, nullptr, err, st));
  }
  return kOk;
}

int launch_cooc_weighted_knn(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                             const int32_t* c2t_idx, int64_t n, int64_t n_cols, const int64_t* wt,
                             const int64_t* queries, int64_t nq, int64_t k, void* scratch, int64_t scratch_bytes,
                             float* out_w, int64_t* out_n, int* err, hipStream_t st) {
  PS_TRY(cooc_check(t2c_ptr, c2t_ptr, n, n_cols, queries, nq));
  PS_REQUIRE(wt != nullptr || n_cols == 0, kErrArg, "cooc: null weights");
  PS_REQUIRE(k >= 1 && k <= n && k <= knn_max_k(), kErrArg, "cooc: need 1 <= k <= min(n_tracks, 4096)");
  PS_REQUIRE((out_w != nullptr && out_n != nullptr) || nq == 0, kErrArg, "cooc: null output");
  if (nq == 0) return kOk;
  PS_REQUIRE(scratch != nullptr && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0, kErrArg,
             "cooc: scratch must be 16-byte aligned");
  // batch of query rows that fits the scratch
  // (a row costs at least n * 4 bytes: start one above that bound and step down)
  int64_t qb = std::min<int64_t>(nq, 65535);
  qb = std::min<int64_t>(qb, std::max<int64_t>(1, scratch_bytes / (n * 4) + 1));
  while (qb > 1 && cooc_weighted_scratch_bytes(n, qb) > scratch_bytes) --qb;
  PS_REQUIRE(cooc_weighted_scratch_bytes(n, qb) <= scratch_bytes, kErrWorkspace, "cooc: scratch too small");
  float* scores = (float*)scratch;
  for (int64_t q0 = 0; q0 < nq; q0 += qb) {
    const int64_t m = std::min(qb, nq - q0);
    PS_TRY(cooc_launch_tiles<CoocScore>(t2c_ptr, t2c_idx, c2t_ptr, c2t_idx, n, n_cols, wt, queries + q0, m, scores,
                                        nullptr, err, st));
    PS_TRY(launch_knn_select_score(scores, n, m, k, out_w + q0 * k, out_n + q0 * k, st));
  }
  return kOk;
}

}  // namespace ps
