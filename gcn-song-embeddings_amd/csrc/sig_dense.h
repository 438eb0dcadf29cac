// sig_dense_kernel: the fused dense term of the full-gradient logistic fits,
//   BIAS form   (lmf.hip):  D = sigmoid(X Y^T + bx + by^T) Y and its row sums
//   WEIGHT form (n2v.hip):  D = (sigmoid(X Y^T) * cw^T) Y, cw a weight per row of Y
// A workgroup of kSigWaves waves owns kSigWaves * 32 rows of X, one 32-row slab
// per wave, and walks Y in tiles of 32 items, ascending.  A tile is staged once
// in LDS (zero-filled past f and past n_other; the next tile's loads are in
// flight in registers while this one is multiplied) and every wave takes it
// twice, both times with the exact-f32 MFMA 32x32x2:
//   S^T (items x rows) = Y_tile X_slab^T.  A = Y_tile from LDS, B = the wave's X
//     slab, held in registers for the whole walk.  Lane half h carries the k
//     values 8q + 4h .. 8q + 4h + 3 of both operands (any assignment of k to the
//     two halves is a valid product as long as A and B agree), so either side is
//     one 16-byte read per four MFMAs.
//   The accumulator has the row of X on the lane and the item in the register:
//     register t of lane half h is item (t & 3) + 8 (t >> 2) + 4h.  Bias (or the
//     column weight), sigmoid and the tail mask are applied there, and in the
//     BIAS form the registers are summed for dsum.
//   D^T (f x rows) += Y_tile^T P^T sums over the item, the accumulator's register
//     index, so register t is the B operand of k-step t as it stands (k = 0 from
//     half 0, k = 1 from half 1); the A operand of that step is the column of Y
//     for the same two items, (t & 3) + 8 (t >> 2) + 4h, read from the LDS tile.
// Rows are MFMA columns, which never mix; items are summed in one fixed order;
// nothing depends on the grid.  The two forms differ in the line that turns a
// score into a probability and in the row sums, nowhere else.  The sparse part
// and the AdaGrad step that consume D are sig_update_kernel (sig_update.h), in
// the same two forms.
#pragma once
#include "rowplan.h"

namespace ps {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kSigWaves = 4;                  // 32-row slabs per workgroup
constexpr int kSigRowBlock = 32 * kSigWaves;  // rows per workgroup
constexpr int kSigTile = 32;                  // items per tile
constexpr int kSigStride = kRowMaxF + 4;      // LDS row stride (floats): 16 rows' 16-byte reads cover 64 banks

// stable logistic function: e = exp(-|s|) never overflows
__device__ __forceinline__ float lmf_sigmoid(float s) {
  const float e = expf(-fabsf(s));
  return (s >= 0.f ? 1.f : e) / (1.f + e);
}

// log(1 + exp(s)) with the same e: -lmf_softplus(-s) is log(lmf_sigmoid(s))
__device__ __forceinline__ float lmf_softplus(float s) { return fmaxf(s, 0.f) + log1pf(expf(-fabsf(s))); }

// WEIGHT form: by is the column weight cw; bx and dsum are unused (null)
struct SigDenseArgs {
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
template <int CB, bool WEIGHT>
__global__ __launch_bounds__(64 * kSigWaves, 2) void sig_dense_kernel(SigDenseArgs A) {
  __shared__ __attribute__((aligned(16))) float Ys[kSigTile * kSigStride];
  __shared__ __attribute__((aligned(16))) float bys[kSigTile];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int f = A.f;
  const int64_t row = (int64_t)blockIdx.x * kSigRowBlock + wv * 32 + r;
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
  float bxr = 0.f;
  if constexpr (!WEIGHT) bxr = live ? A.bx[row] : 0.f;

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
      const int s = tid + 64 * kSigWaves * j;
      const int64_t gi = i0 + s / (8 * CB);
      const int c = 4 * (s % (8 * CB));
      pre[j] = gi < A.n_other && c < f ? *reinterpret_cast<const float4*>(A.Y + gi * A.ldy + c)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < kSigTile) preb = i0 + tid < A.n_other ? A.by[i0 + tid] : 0.f;
  };
  fetch(0);

  for (int64_t i0 = 0; i0 < A.n_other; i0 += kSigTile) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int s = tid + 64 * kSigWaves * j;
      *reinterpret_cast<float4*>(Ys + (s / (8 * CB)) * kSigStride + 4 * (s % (8 * CB))) = pre[j];
    }
    if (tid < kSigTile) bys[tid] = preb;
    __syncthreads();
    if (i0 + kSigTile < A.n_other) fetch(i0 + kSigTile);

    f32x16 sc;
#pragma unroll
    for (int t = 0; t < 16; ++t) sc[t] = 0.f;
#pragma unroll
    for (int q = 0; q < 4 * CB; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(Ys + r * kSigStride + 8 * q + 4 * h);
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
        float p;
        if constexpr (WEIGHT) p = bb[j] * lmf_sigmoid(sc[4 * g + j]);
        else p = lmf_sigmoid((sc[4 * g + j] + bxr) + bb[j]);
        const float pm = i0 + 8 * g + 4 * h + j < A.n_other ? p : 0.f;
        sc[4 * g + j] = pm;
        if constexpr (!WEIGHT) psum += pm;
      }
    }

#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float a = Ys[((t & 3) + 8 * (t >> 2) + 4 * h) * kSigStride + 32 * cb + r];
        dacc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sc[t], dacc[cb], 0, 0, 0);
      }
    }
  }

  // D^T: the row of X on the lane, column 32 cb + 8g + 4h + j in register 4g + j
  float ptot = 0.f;
  if constexpr (!WEIGHT) ptot = psum + __shfl_xor(psum, 32, 64);
  if (live) {
    if constexpr (!WEIGHT)
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

template <bool WEIGHT>
inline void sig_dense_launch(const SigDenseArgs& A, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(A.n_rows, kSigRowBlock)), block(64 * kSigWaves);
  switch (ceil_div(A.f, 32)) {
    case 1: hipLaunchKernelGGL((sig_dense_kernel<1, WEIGHT>), grid, block, 0, st, A); break;
    case 2: hipLaunchKernelGGL((sig_dense_kernel<2, WEIGHT>), grid, block, 0, st, A); break;
    case 3: hipLaunchKernelGGL((sig_dense_kernel<3, WEIGHT>), grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL((sig_dense_kernel<4, WEIGHT>), grid, block, 0, st, A); break;
  }
}

}  // namespace ps
