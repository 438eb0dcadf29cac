// Implicit-feedback alternating least squares (Hu, Koren, Volinsky) with the
// conjugate-gradient row solve of Takacs et al.: the fit behind the reference's
// ColTrackCfALS / TrackTrackCfALS baselines (baselines.py:458-514), which takes
// it from implicit.cpu.als.  The arithmetic is this project's definition (als.h);
// no parity with that package is claimed.
//
// gram_kernel: G = Y^T Y + reg I.  A workgroup owns an 8 x 8 tile of G; its 16
// waves each take every 16th row of Y into a private running sum (fma, rows
// ascending) and the 16 partial sums are added in wave order: a fixed order, no
// atomics, and G[a][b] and G[b][a] are the same bits.
//
// als_half_kernel: one half-iteration on the row plan of rowplan.h (the item
// walk, the long row's wave-order sum, the dispatch of a block of rows).  A
// workgroup stages G in LDS once (64 KiB at f = 128: two workgroups per CU) and
// walks kAlsBlocks blocks of rows.  The lane's two columns hold x, r, p, Ap and
// a gathered y_i alike: G p is f steps of one LDS read (row k of G,
// conflict-free) against p[k] read from its lane, and a dot product is a lane
// product and the xor butterfly, whose result is the same in every lane.  In a
// long row every wave carries the same x, r, p (same inputs, same instructions:
// same bits); only the item sums are split.
#include <algorithm>

#include "als.h"
#include "rowplan.h"

namespace ps {

constexpr int kAlsBlocks = 4;       // blocks of rows per workgroup: G is staged once per 32 rows
constexpr float kAlsTiny = 1e-20f;  // a squared residual below this ends the row's solve

constexpr int kGramTile = 8;
constexpr int kGramSlices = 16;

__global__ __launch_bounds__(64 * kGramSlices) void gram_kernel(const float* __restrict__ Y, int64_t n, int f,
                                                                 int64_t ld, float reg, float* __restrict__ G) {
  __shared__ float part[kGramSlices][64];
  const int t = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int a = blockIdx.y * kGramTile + (t >> 3), b = blockIdx.x * kGramTile + (t & 7);
  const bool on = a < f && b < f;
  float acc = 0.f;
  if (on) {
#pragma unroll 4
    for (int64_t i = s; i < n; i += kGramSlices) acc = fmaf(Y[i * ld + a], Y[i * ld + b], acc);
  }
  part[s][t] = acc;
  __syncthreads();
  if (s == 0 && on) {
    float v = part[0][t];
#pragma unroll
    for (int k = 1; k < kGramSlices; ++k) v += part[k][t];
    if (a == b) v += reg;
    G[(int64_t)a * f + b] = v;
  }
}

struct AlsArgs {
  const int64_t* ptr;
  int64_t n_rows;
  RowItems I;  // by unused
  float* X;
  int64_t ldx;
  int f;
  int steps;
};

__device__ __forceinline__ float als_dot(float2 a, float2 b) { return wave_sum(fmaf(a.x, b.x, a.y * b.y)); }

// (G v)[c] = sum_k G[k][c] v[k], k ascending, for the lane's two columns
__device__ __forceinline__ float2 als_gv(const float* __restrict__ Gs, int f, int c0, float2 v) {
  float2 acc = make_float2(0.f, 0.f);
  for (int k = 0; k < f; k += 2) {
    const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), k >> 1));
    const float v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), k >> 1));
    const float2 g0 = *reinterpret_cast<const float2*>(Gs + k * f + c0);
    const float2 g1 = *reinterpret_cast<const float2*>(Gs + (k + 1) * f + c0);
    acc.x = fmaf(g0.x, v0, acc.x);
    acc.y = fmaf(g0.y, v0, acc.y);
    acc.x = fmaf(g1.x, v1, acc.x);
    acc.y = fmaf(g1.y, v1, acc.y);
  }
  return acc;
}

// sum over the row's items [b, e) of
//   RES:  (c - (c - 1) (y . v)) y      else:  (c - 1) (y . v) y,     c = alpha val
// LONG: called by every wave of the workgroup with the same v; barriers inside.
template <bool RES, bool LONG>
__device__ __forceinline__ float2 als_sum(const AlsArgs& A, int64_t b, int64_t e, int lane, int wv, int c0, bool on,
                                          float* __restrict__ part, float2 v) {
  float2 acc = make_float2(0.f, 0.f);
  row_walk<false>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                  [&](float2 y, float cu, float) __attribute__((always_inline)) {
                    const float d = als_dot(y, v);
                    const float w = RES ? cu - (cu - 1.f) * d : (cu - 1.f) * d;
                    acc.x = fmaf(w, y.x, acc.x);
                    acc.y = fmaf(w, y.y, acc.y);
                  });
  if constexpr (LONG) {
    float none = 0.f;
    acc = row_wave_order_sum<true, false>(part, A.f, nullptr, lane, wv, c0, on, acc, none);
  }
  return acc;
}

template <bool LONG>
__device__ __forceinline__ void als_row(const AlsArgs& A, int64_t row, const float* __restrict__ Gs,
                                        float* __restrict__ part, int lane, int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float2 x = row_ld2(xr, on);
  const float2 s = als_sum<true, LONG>(A, b, e, lane, wv, c0, on, part, x);
  const float2 g = als_gv(Gs, f, c0, x);
  float2 r = make_float2(on ? s.x - g.x : 0.f, on ? s.y - g.y : 0.f);
  float2 p = r;
  float rs = als_dot(r, r);
  if (rs < kAlsTiny) return;  // the same in every lane (and, LONG, in every wave)
  for (int it = 0; it < A.steps; ++it) {
    const float2 si = als_sum<false, LONG>(A, b, e, lane, wv, c0, on, part, p);
    const float2 gp = als_gv(Gs, f, c0, p);
    const float2 Ap = make_float2(on ? gp.x + si.x : 0.f, on ? gp.y + si.y : 0.f);
    const float a = rs / als_dot(p, Ap);
    x.x = fmaf(a, p.x, x.x);
    x.y = fmaf(a, p.y, x.y);
    r.x = fmaf(-a, Ap.x, r.x);
    r.y = fmaf(-a, Ap.y, r.y);
    const float rn = als_dot(r, r);
    if (rn < kAlsTiny) break;
    const float beta = rn / rs;
    p.x = fmaf(beta, p.x, r.x);
    p.y = fmaf(beta, p.y, r.y);
    rs = rn;
  }
  if (on && (!LONG || wv == 0)) *reinterpret_cast<float2*>(xr) = x;
}

__global__ __launch_bounds__(64 * kRowWaves) void als_half_kernel(AlsArgs A, const float* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) float als_lds[];
  float* Gs = als_lds;               // [f][f]
  float* part = als_lds + A.f * A.f;  // [kRowWaves][f]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < A.f * A.f / 4; i += 64 * kRowWaves)
    reinterpret_cast<float4*>(Gs)[i] = reinterpret_cast<const float4*>(G)[i];
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * (kAlsBlocks * kRowWaves);
  const int64_t last = min<int64_t>(A.n_rows, first + kAlsBlocks * kRowWaves);
  for (int64_t r0 = first; r0 < last; r0 += kRowWaves)
    row_block(
        A.ptr, A.n_rows, r0, wv,
        [&](int64_t row) __attribute__((always_inline)) { als_row<false>(A, row, Gs, part, lane, wv); },
        [&](int64_t row) __attribute__((always_inline)) { als_row<true>(A, row, Gs, part, lane, wv); });
}

int als_rows_per_block() { return kRowWaves; }
int als_long_row() { return kRowLong; }

int launch_als_gram(const float* Y, int64_t n, int64_t f, int64_t ld, float reg, float* G, hipStream_t st) {
  PS_TRY(row_tables_ok("als_gram", f, {{"Y", Y, ld}}));
  PS_REQUIRE(G != nullptr && (reinterpret_cast<uintptr_t>(G) & 15) == 0, kErrArg, "als_gram: G must be 16-byte aligned");
  PS_REQUIRE(n >= 0 && n <= INT32_MAX, kErrArg, "als_gram: bad row count");
  PS_REQUIRE(reg > 0.f, kErrArg, "als_gram: reg must be positive");  // false for NaN too
  const unsigned tiles = (unsigned)ceil_div(f, kGramTile);
  hipLaunchKernelGGL(gram_kernel, dim3(tiles, tiles), dim3(64 * kGramSlices), 0, st, Y, n, (int)f, ld, reg, G);
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_als_half(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                    int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* G, float alpha,
                    int64_t cg_steps, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("als_half", f, {{"Y", Y, ldy}, {"X", X, ldx}}));
  PS_REQUIRE(G != nullptr && (reinterpret_cast<uintptr_t>(G) & 15) == 0, kErrArg, "als_half: G must be 16-byte aligned");
  PS_REQUIRE(ptr != nullptr, kErrArg, "als_half: null row pointers");
  PS_TRY(row_sizes_ok("als_half", n_rows, n_other));
  PS_REQUIRE(cg_steps >= 0 && cg_steps <= INT32_MAX, kErrArg, "als_half: cg_steps must be >= 0");
  PS_REQUIRE(alpha > 0.f && alpha < INFINITY, kErrArg, "als_half: alpha must be positive and finite");
  if (n_rows == 0 || cg_steps == 0) return kOk;  // zero steps leave X as it is
  const int lds = (int)((f * f + kRowWaves * f) * 4);
  static int prepared = 0;
  if (!prepared) {
    PS_CHECK_HIP(hipFuncSetAttribute((const void*)als_half_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (kRowMaxF * kRowMaxF + kRowWaves * kRowMaxF) * 4));
    prepared = 1;
  }
  // A workgroup per kAlsBlocks blocks of rows, not a resident grid striding over all of them: the
  // dispatcher hands the next workgroup to whichever CU has room, so the one that met a hub row is
  // not left with an equal share of the other rows as well.
  const int grid = ceil_div(n_rows, kAlsBlocks * kRowWaves);
  const AlsArgs A{ptr, n_rows, {idx, val, alpha, Y, nullptr, n_other, ldy, err}, X, ldx, (int)f, (int)cg_steps};
  hipLaunchKernelGGL(als_half_kernel, dim3((unsigned)grid), dim3(64 * kRowWaves), lds, st, A, G);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
