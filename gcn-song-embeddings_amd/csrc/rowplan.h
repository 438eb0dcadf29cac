// The row plan of the row-wise fits' kernels (als_half_kernel in als.hip,
// sig_update_kernel in sig_update.h for lmf.hip and n2v.hip, the two kernels of
// bpr.hip): a workgroup of kRowWaves
// waves owns a block of kRowWaves consecutive CSR rows.  A lane owns columns
// 2 lane and 2 lane + 1 of every f-vector, so a gathered row of Y is one 8-byte
// load per lane.  An ordinary row (at most kRowLong items) is one wave's, its
// items in CSR order; a long row is the whole workgroup's, wave w taking the
// 64-item groups w, w + kRowWaves, ... and the kRowWaves partial sums meeting in
// LDS, added in wave order.  Which form a row takes depends on its length alone
// and neither form's sum order depends on the grid.  The id clamp, the gather
// loop and the wave-order sum are written here and nowhere else.
#pragma once
#include <initializer_list>

#include "common.h"

namespace ps {

constexpr int kRowWaves = 8;     // waves (= ordinary rows) per workgroup and block of rows
constexpr int kRowInFlight = 8;  // item rows whose loads are in flight per step
constexpr int kRowLong = 512;    // a row above this many items is taken by the workgroup
constexpr int kRowMaxF = 128;    // 2 columns per lane

// the items' side of a half-iteration; by is read by a walk with BIAS only
struct RowItems {
  const int32_t* idx;
  const float* val;
  float alpha;
  const float* Y;
  const float* by;
  int64_t n_other, ldy;
  int* err;
};

__device__ __forceinline__ float2 row_ld2(const float* p, bool on) {
  return on ? *reinterpret_cast<const float2*>(p) : make_float2(0.f, 0.f);
}

// whether id v is in the ascending row [b, e) of idx
__device__ __forceinline__ bool row_holds(const int32_t* __restrict__ idx, int64_t b, int64_t e, int32_t v) {
  while (b < e) {
    const int64_t m = b + ((e - b) >> 1);
    const int32_t a = idx[m];
    if (a == v) return true;
    if (a < v) b = m + 1;
    else e = m;
  }
  return false;
}

// The items [b, e) in groups of 64 (group g0, g0 + gs, ...), in order:
// use(y_i, alpha val_i, BIAS ? by[i] : 0) with the lane's two columns of y_i.
template <bool BIAS, class Use>
__device__ __forceinline__ void row_walk(const RowItems& I, int64_t b, int64_t e, int g0, int gs, int lane, int c0,
                                         bool on, Use use) {
  for (int64_t j0 = b + (int64_t)g0 * 64; j0 < e; j0 += (int64_t)gs * 64) {  // wave-uniform
    const int m = (int)min<int64_t>(64, e - j0);
    int id = 0;
    float c = 0.f, bi = 0.f;
    if (lane < m) {
      id = I.idx[j0 + lane];
      if (id < 0 || id >= I.n_other) {  // callers validate; clamp so that no access strays
        if (I.err) atomicExch(I.err, 1);
        id = 0;
      }
      c = I.alpha * I.val[j0 + lane];
      if constexpr (BIAS) bi = I.by[id];
    }
    int u = 0;
    for (; u + kRowInFlight <= m; u += kRowInFlight) {
      float2 y[kRowInFlight];
      float cu[kRowInFlight], bu[kRowInFlight];
#pragma unroll
      for (int r = 0; r < kRowInFlight; ++r) {
        y[r] = row_ld2(I.Y + (int64_t)__shfl(id, u + r, 64) * I.ldy + c0, on);
        cu[r] = __shfl(c, u + r, 64);
        bu[r] = BIAS ? __shfl(bi, u + r, 64) : 0.f;
      }
#pragma unroll
      for (int r = 0; r < kRowInFlight; ++r) use(y[r], cu[r], bu[r]);
    }
    for (; u < m; ++u)
      use(row_ld2(I.Y + (int64_t)__shfl(id, u, 64) * I.ldy + c0, on), __shfl(c, u, 64),
          BIAS ? __shfl(bi, u, 64) : 0.f);
  }
}

// A long row's sum, called by every wave of the workgroup (two barriers inside):
// wave w leaves its partial sum at part + w stride (SCALAR: and sc at spart[w]);
// the kRowWaves of them are added in wave order from wave 0's value.  The sum is
// returned (sc replaced) in every wave if ALL, else in wave 0 only.
template <bool ALL, bool SCALAR>
__device__ __forceinline__ float2 row_wave_order_sum(float* __restrict__ part, int stride, float* __restrict__ spart,
                                                     int lane, int wv, int c0, bool on, float2 mine, float& sc) {
  if (on) *reinterpret_cast<float2*>(part + wv * stride + c0) = mine;
  if (SCALAR && lane == 0) spart[wv] = sc;
  __syncthreads();
  float2 s = make_float2(0.f, 0.f);
  if (ALL || wv == 0) {
    if (on) {
      s = *reinterpret_cast<const float2*>(part + c0);
#pragma unroll
      for (int w = 1; w < kRowWaves; ++w) {
        const float2 t = *reinterpret_cast<const float2*>(part + w * stride + c0);
        s.x += t.x;
        s.y += t.y;
      }
    }
    if (SCALAR) {
      sc = spart[0];
#pragma unroll
      for (int w = 1; w < kRowWaves; ++w) sc += spart[w];
    }
  }
  __syncthreads();  // part is free again
  return s;
}

// The block of rows r0 .. r0 + kRowWaves - 1: row r0 + wv by this wave if it is
// ordinary, then the block's long rows one after another, each by all waves
// (workgroup-uniform: by_workgroup may hold barriers).
template <class Wave, class Workgroup>
__device__ __forceinline__ void row_block(const int64_t* __restrict__ ptr, int64_t n_rows, int64_t r0, int wv,
                                          Wave by_wave, Workgroup by_workgroup) {
  const int64_t row = r0 + wv;
  if (row < n_rows && ptr[row + 1] - ptr[row] <= kRowLong) by_wave(row);
  for (int w = 0; w < kRowWaves; ++w) {
    const int64_t lr = r0 + w;
    if (lr < n_rows && ptr[lr + 1] - ptr[lr] > kRowLong) by_workgroup(lr);
  }
}

inline bool row_table_ok(const float* t, int64_t f, int64_t ld) {
  return t != nullptr && (reinterpret_cast<uintptr_t>(t) & 15) == 0 && ld >= f && ld % 4 == 0;
}

// the refusals every launcher `who` makes of f and of its f-column tables
struct RowTable {
  const char* name;
  const float* t;
  int64_t ld;
};
inline int row_tables_ok(const std::string& who, int64_t f, std::initializer_list<RowTable> tables) {
  PS_REQUIRE(f >= 4 && f <= kRowMaxF && f % 4 == 0, kErrArg, who + ": need 4 <= f <= 128, f % 4 == 0");
  for (const RowTable& t : tables)
    PS_REQUIRE(row_table_ok(t.t, f, t.ld), kErrArg,
               who + ": " + t.name + " must be 16-byte aligned with ld >= f, ld % 4 == 0");
  return kOk;
}
inline int row_sizes_ok(const std::string& who, int64_t n_rows, int64_t n_other) {
  PS_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX && n_other >= 1 && n_other <= INT32_MAX, kErrArg,
             who + ": bad sizes");
  return kOk;
}

}  // namespace ps
