// Logistic matrix factorisation, full-gradient AdaGrad ascent (definition: lmf.h).
//
// lmf_dense_kernel: D = sigmoid(X Y^T + bx + by^T) Y and its row sums, fused.  A
// workgroup of kLmfWaves waves owns kLmfWaves * 32 rows of X, one 32-row slab per
// wave, and walks Y in tiles of 32 items, ascending.  A tile is staged once in
// LDS (zero-filled past f and past n_other; the next tile's loads are in flight
// in registers while this one is multiplied) and every wave takes it twice, both
// times with the exact-f32 MFMA 32x32x2:
//   S^T (items x rows) = Y_tile X_slab^T.  A = Y_tile from LDS, B = the wave's X
//     slab, held in registers for the whole walk.  Lane half h carries the k
//     values 8q + 4h .. 8q + 4h + 3 of both operands (any assignment of k to the
//     two halves is a valid product as long as A and B agree), so either side is
//     one 16-byte read per four MFMAs.
//   The accumulator has the row of X on the lane and the item in the register:
//     register t of lane half h is item (t & 3) + 8 (t >> 2) + 4h.  Bias, sigmoid
//     and the tail mask are applied there, and the registers are summed for dsum.
//   D^T (f x rows) += Y_tile^T P^T sums over the item, the accumulator's register
//     index, so register t is the B operand of k-step t as it stands (k = 0 from
//     half 0, k = 1 from half 1); the A operand of that step is the column of Y
//     for the same two items, (t & 3) + 8 (t >> 2) + 4h, read from the LDS tile.
// Rows are MFMA columns, which never mix; items are summed in one fixed order;
// nothing depends on the grid.
//
// lmf_update_kernel: the sparse part and the AdaGrad step on the row plan of
// rowplan.h, one wave per row, the workgroup for a long row: the walk also
// gathers by[i] and carries the scalar sum of w_i, and wave 0 finishes a long row.
#include <algorithm>
#include <cmath>

#include "lmf.h"
#include "rowplan.h"

namespace ps {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kLmfWaves = 4;                  // dense: 32-row slabs per workgroup
constexpr int kLmfRowBlock = 32 * kLmfWaves;  // dense: rows per workgroup
constexpr int kLmfTile = 32;                  // dense: items per tile
constexpr int kLmfStride = kRowMaxF + 4;      // dense: LDS row stride (floats): 16 rows' 16-byte reads cover 64 banks
constexpr float kLmfEps = 1e-6f;

// stable logistic function: e = exp(-|s|) never overflows
__device__ __forceinline__ float lmf_sigmoid(float s) {
  const float e = expf(-fabsf(s));
  return (s >= 0.f ? 1.f : e) / (1.f + e);
}

struct LmfDenseArgs {
  const float* X;
  const float* bx;
  int64_t n_rows, ldx;
  const float* Y;
  const float* by;
  int64_t n_other, ldy;
  int f;
  float* D;
  int64_t ldd;
  float* dsum;
};

// CB = ceil(f / 32): blocks of 32 columns;
// two workgroups per CU: at CB = 4 the compiler otherwise settles on 267 registers and one wave per SIMD
template <int CB>
__global__ __launch_bounds__(64 * kLmfWaves, 2) void lmf_dense_kernel(LmfDenseArgs A) {
  __shared__ __attribute__((aligned(16))) float Ys[kLmfTile * kLmfStride];
  __shared__ __attribute__((aligned(16))) float bys[kLmfTile];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int f = A.f;
  const int64_t row = (int64_t)blockIdx.x * kLmfRowBlock + wv * 32 + r;
  const bool live = row < A.n_rows;

  // B operand of the first product: x[8q + 4h + j] in xf[4q + j]
  float xf[16 * CB];
#pragma unroll
  for (int q = 0; q < 4 * CB; ++q) {
    const int k = 8 * q + 4 * h;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && k < f) v = *reinterpret_cast<const float4*>(A.X + row * A.ldx + k);
    xf[4 * q] = v.x;
    xf[4 * q + 1] = v.y;
    xf[4 * q + 2] = v.z;
    xf[4 * q + 3] = v.w;
  }
  const float bxr = live ? A.bx[row] : 0.f;

  f32x16 dacc[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int t = 0; t < 16; ++t) dacc[cb][t] = 0.f;
  float psum = 0.f;

  // the tile is 32 items x 8 CB float4: CB per thread
  float4 pre[CB];
  float preb = 0.f;
  auto fetch = [&](int64_t i0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int s = tid + 64 * kLmfWaves * j;
      const int64_t gi = i0 + s / (8 * CB);
      const int c = 4 * (s % (8 * CB));
      pre[j] = gi < A.n_other && c < f ? *reinterpret_cast<const float4*>(A.Y + gi * A.ldy + c)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < kLmfTile) preb = i0 + tid < A.n_other ? A.by[i0 + tid] : 0.f;
  };
  fetch(0);

  for (int64_t i0 = 0; i0 < A.n_other; i0 += kLmfTile) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int s = tid + 64 * kLmfWaves * j;
      *reinterpret_cast<float4*>(Ys + (s / (8 * CB)) * kLmfStride + 4 * (s % (8 * CB))) = pre[j];
    }
    if (tid < kLmfTile) bys[tid] = preb;
    __syncthreads();
    if (i0 + kLmfTile < A.n_other) fetch(i0 + kLmfTile);

    f32x16 sc;
#pragma unroll
    for (int t = 0; t < 16; ++t) sc[t] = 0.f;
#pragma unroll
    for (int q = 0; q < 4 * CB; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(Ys + r * kLmfStride + 8 * q + 4 * h);
      sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xf[4 * q], sc, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xf[4 * q + 1], sc, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xf[4 * q + 2], sc, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xf[4 * q + 3], sc, 0, 0, 0);
    }

    // registers 4g .. 4g + 3 are items 8g + 4h .. 8g + 4h + 3 of the tile.  A tail item's
    // sigmoid(0 + biases) is not zero: mask the probability, not only the loads.
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b = *reinterpret_cast<const float4*>(bys + 8 * g + 4 * h);
      const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = lmf_sigmoid((sc[4 * g + j] + bxr) + bb[j]);
        const float pm = i0 + 8 * g + 4 * h + j < A.n_other ? p : 0.f;
        sc[4 * g + j] = pm;
        psum += pm;
      }
    }

#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float a = Ys[((t & 3) + 8 * (t >> 2) + 4 * h) * kLmfStride + 32 * cb + r];
        dacc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sc[t], dacc[cb], 0, 0, 0);
      }
    }
  }

  // D^T: the row of X on the lane, column 32 cb + 8g + 4h + j in register 4g + j
  const float ptot = psum + __shfl_xor(psum, 32, 64);
  if (live) {
    if (h == 0) A.dsum[row] = ptot;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * cb + 8 * g + 4 * h;
        if (c < f)
          *reinterpret_cast<float4*>(A.D + row * A.ldd + c) =
              make_float4(dacc[cb][4 * g], dacc[cb][4 * g + 1], dacc[cb][4 * g + 2], dacc[cb][4 * g + 3]);
      }
    }
  }
}

struct LmfUpArgs {
  const int64_t* ptr;
  int64_t n_rows;
  RowItems I;
  float* X;
  float* bx;
  int64_t ldx;
  int f;
  const float* D;
  int64_t ldd;
  const float* dsum;
  float* H;
  int64_t ldh;
  float* hb;
  float reg, lr;
};

// LONG: called by every wave of the workgroup; barriers inside.
template <bool LONG>
__device__ __forceinline__ void lmf_row(const LmfUpArgs& A, int64_t row, float* __restrict__ part, int lane, int wv) {
  const int f = A.f, c0 = 2 * lane < f ? 2 * lane : 0;
  const bool on = 2 * lane < f;
  const int64_t b = A.ptr[row], e = A.ptr[row + 1];
  float* xr = A.X + row * A.ldx + c0;
  float* hr = A.H + row * A.ldh + c0;
  const float2 x = row_ld2(xr, on);
  const float bxu = A.bx[row];
  // the sums over the row's items of w_i y_i, and of w_i
  float2 acc = make_float2(0.f, 0.f);
  float ws = 0.f;
  row_walk<true>(A.I, b, e, LONG ? wv : 0, LONG ? kRowWaves : 1, lane, c0, on,
                 [&](float2 y, float cu, float bu) __attribute__((always_inline)) {
                   const float s = (wave_sum(fmaf(x.x, y.x, x.y * y.y)) + bxu) + bu;
                   const float w = cu * lmf_sigmoid(-s);
                   acc.x = fmaf(w, y.x, acc.x);
                   acc.y = fmaf(w, y.y, acc.y);
                   ws += w;
                 });
  if constexpr (LONG) {
    acc = row_wave_order_sum<false, true>(part, kRowMaxF, part + kRowWaves * kRowMaxF, lane, wv, c0, on, acc, ws);
    if (wv != 0) return;  // wave 0 has the sums and finishes the row
  }
  const float2 s = acc;
  if (on) {
    const float2 d = *reinterpret_cast<const float2*>(A.D + row * A.ldd + c0);
    float2 hh = *reinterpret_cast<const float2*>(hr);
    const float gx = fmaf(-A.reg, x.x, s.x - d.x), gy = fmaf(-A.reg, x.y, s.y - d.y);
    hh.x = fmaf(gx, gx, hh.x);
    hh.y = fmaf(gy, gy, hh.y);
    *reinterpret_cast<float2*>(hr) = hh;
    if (A.lr != 0.f)
      *reinterpret_cast<float2*>(xr) =
          make_float2(x.x + A.lr * gx / sqrtf(kLmfEps + hh.x), x.y + A.lr * gy / sqrtf(kLmfEps + hh.y));
  }
  if (lane == 0) {
    const float gb = ws - A.dsum[row];
    const float hn = fmaf(gb, gb, A.hb[row]);
    A.hb[row] = hn;
    if (A.lr != 0.f) A.bx[row] = bxu + A.lr * gb / sqrtf(kLmfEps + hn);
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void lmf_update_kernel(LmfUpArgs A) {
  __shared__ __attribute__((aligned(16))) float part[kRowWaves * kRowMaxF + kRowWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  row_block(
      A.ptr, A.n_rows, (int64_t)blockIdx.x * kRowWaves, wv,
      [&](int64_t row) __attribute__((always_inline)) { lmf_row<false>(A, row, part, lane, wv); },
      [&](int64_t row) __attribute__((always_inline)) { lmf_row<true>(A, row, part, lane, wv); });
}

int lmf_row_block() { return kLmfRowBlock; }
int lmf_long_row() { return kRowLong; }

int launch_lmf_dense(const float* X, const float* bx, int64_t n_rows, int64_t ldx, const float* Y, const float* by,
                     int64_t n_other, int64_t ldy, int64_t f, float* D, int64_t ldd, float* dsum, hipStream_t st) {
  PS_TRY(row_tables_ok("lmf_dense", f, {{"X", X, ldx}, {"Y", Y, ldy}, {"D", D, ldd}}));
  PS_REQUIRE(bx != nullptr && by != nullptr && dsum != nullptr, kErrArg, "lmf_dense: null bias or dsum");
  PS_TRY(row_sizes_ok("lmf_dense", n_rows, n_other));
  if (n_rows == 0) return kOk;
  const LmfDenseArgs A{X, bx, n_rows, ldx, Y, by, n_other, ldy, (int)f, D, ldd, dsum};
  const dim3 grid((unsigned)ceil_div(n_rows, kLmfRowBlock)), block(64 * kLmfWaves);
  switch (ceil_div(f, 32)) {
    case 1: hipLaunchKernelGGL(lmf_dense_kernel<1>, grid, block, 0, st, A); break;
    case 2: hipLaunchKernelGGL(lmf_dense_kernel<2>, grid, block, 0, st, A); break;
    case 3: hipLaunchKernelGGL(lmf_dense_kernel<3>, grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL(lmf_dense_kernel<4>, grid, block, 0, st, A); break;
  }
  PS_CHECK_LAUNCH();
  return kOk;
}

int launch_lmf_update(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                      const float* by, int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f,
                      const float* D, int64_t ldd, const float* dsum, float* H, int64_t ldh, float* hb, float alpha,
                      float reg, float lr, int* err, hipStream_t st) {
  PS_TRY(row_tables_ok("lmf_update", f, {{"Y", Y, ldy}, {"X", X, ldx}, {"D", D, ldd}, {"H", H, ldh}}));
  PS_REQUIRE(ptr != nullptr && by != nullptr && bx != nullptr && dsum != nullptr && hb != nullptr, kErrArg,
             "lmf_update: null row pointers, bias, dsum or hb");
  PS_TRY(row_sizes_ok("lmf_update", n_rows, n_other));
  PS_REQUIRE(alpha > 0.f && alpha < INFINITY, kErrArg, "lmf_update: alpha must be positive and finite");
  PS_REQUIRE(reg >= 0.f && reg < INFINITY && lr >= 0.f && lr < INFINITY, kErrArg,
             "lmf_update: reg and lr must be non-negative and finite");
  if (n_rows == 0) return kOk;
  const LmfUpArgs A{ptr, n_rows, {idx, val, alpha, Y, by, n_other, ldy, err}, X, bx, ldx, (int)f, D, ldd, dsum, H, ldh,
                    hb, reg, lr};
  hipLaunchKernelGGL(lmf_update_kernel, dim3((unsigned)ceil_div(n_rows, kRowWaves)), dim3(64 * kRowWaves), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
