// Segmented weighted mean: the MEAN aggregator of lib/gnns
// (GNNs_unsupervised.py:537-588, GNN_model.aggregate with agg_func 'MEAN').
// The reference builds a dense [F, U] mask (ones at each sampled neighbour,
// times sqrt(edge count), L1-normalised by F.normalize(p=1)) and multiplies it
// with the [U, d] embedding matrix; the mask has a handful of non-zeros per
// row, so here it is a CSR (seg_ptr, cols, w) and the product is a per-row
// gather-and-accumulate: HBM-bound, one wave per row, float4 column chunks per
// lane, four neighbour rows' loads in flight per step.  The backward of the
// product (dH = mask^T dOut) is the same kernel over the transposed CSR with
// the normalisation already folded into its weights (normalize = 0), so no
// atomics and a fixed summation order.
//
// The GAT aggregator (gat=True of the same function) follows below: gnns.h has
// its definitions and summation orders.
#include "../../include/pinsage_hip.h"
#include "gnns.h"

namespace ps {

// out[i, :] = sum_j w_j * h[cols_j, :] / den_i,  den_i = max(sum_j |w_j|, 1e-12)
// (normalize) or 1.  Rows whose neighbours are out of [0, n_h) skip them, in
// the sum and in den_i.
template <bool VEC>
__global__ __launch_bounds__(256) void segment_wmean_kernel(
    const float* __restrict__ h, int64_t ldh, int64_t n_h, int d, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ cols, const float* __restrict__ w, int64_t n_seg, int normalize,
    float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_seg) return;
  const int64_t b = seg_ptr[row], e = seg_ptr[row + 1];
  float inv = 1.f;
  if (normalize) {
    float s = 0.f;
    for (int64_t j = b + lane; j < e; j += 64)
      if ((uint64_t)(int64_t)cols[j] < (uint64_t)n_h) s += fabsf(w[j]);  // (a skipped neighbour has no weight)
    s = wave_sum(s);
    inv = 1.f / fmaxf(s, 1e-12f);
  }
  float* o = out + row * ldo;
  if constexpr (VEC) {
    for (int c = 4 * lane; c < d; c += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int64_t j = b;
      for (; j + 4 <= e; j += 4) {
        float4 x[4];
        float wj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t r = cols[j + u];
          const bool ok = (uint64_t)r < (uint64_t)n_h;
          wj[u] = ok ? w[j + u] * inv : 0.f;
          x[u] = *reinterpret_cast<const float4*>(h + (ok ? r : 0) * ldh + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc.x = fmaf(wj[u], x[u].x, acc.x);
          acc.y = fmaf(wj[u], x[u].y, acc.y);
          acc.z = fmaf(wj[u], x[u].z, acc.z);
          acc.w = fmaf(wj[u], x[u].w, acc.w);
        }
      }
      for (; j < e; ++j) {
        const int64_t r = cols[j];
        if ((uint64_t)r >= (uint64_t)n_h) continue;
        const float wj = w[j] * inv;
        const float4 x = *reinterpret_cast<const float4*>(h + r * ldh + c);
        acc.x = fmaf(wj, x.x, acc.x);
        acc.y = fmaf(wj, x.y, acc.y);
        acc.z = fmaf(wj, x.z, acc.z);
        acc.w = fmaf(wj, x.w, acc.w);
      }
      *reinterpret_cast<float4*>(o + c) = acc;
    }
  } else {
    for (int c = lane; c < d; c += 64) {
      float acc = 0.f;
      for (int64_t j = b; j < e; ++j) {
        const int64_t r = cols[j];
        if ((uint64_t)r >= (uint64_t)n_h) continue;
        acc = fmaf(w[j] * inv, h[r * ldh + c], acc);
      }
      o[c] = acc;
    }
  }
}

// ---------------------------------------------------------------- GAT (gnns.h)
__device__ __forceinline__ float lane_bcast(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

struct GatEdge {
  float e, m;
  bool keep;
};
// Score of one entry: sl = s_l[own] (own_ok: own is a row of h), r = hrow_j.
__device__ __forceinline__ GatEdge gat_edge(float sl, bool own_ok, const float* __restrict__ s_r, int32_t r,
                                            int64_t n_h, float c) {
// m is a rounded product: were the multiplication fused into the m - M that
// follows in one pass and not in another, the p of a segment would not sum to
// 1 (an error of half an ulp of m per entry, 8e-6 at |m| = 200).
#pragma clang fp contract(off)
  GatEdge g;
  const bool ok = own_ok && (uint64_t)(int64_t)r < (uint64_t)n_h;
  g.e = ok ? sl + s_r[r] : 0.f;
  g.m = (g.e > 0.f ? g.e : kGatSlope * g.e) * c;
  g.keep = ok && g.m != 0.f;
  return g;
}

// acc += sum_{u < cnt} w_u * src[r_u][c ..] in order of u, where lane u holds
// (w_u, r_u) and every r_u is a row of src.  The broadcasts run with all lanes
// active; act (this lane has columns at c) only guards the loads.  Four rows'
// loads are in flight per step.  VEC: float4 at c; otherwise acc.x at c.
template <bool VEC>
__device__ __forceinline__ void chunk_gather(const float* __restrict__ src, int64_t ld, int c, bool act, float wl,
                                             int32_t rl, int cnt, float4& acc) {
  int u = 0;
  for (; u + 4 <= cnt; u += 4) {
    float wj[4];
    int64_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wj[k] = lane_bcast(wl, u + k);
      r[k] = __builtin_amdgcn_readlane(rl, u + k);
    }
    if (act) {
      if constexpr (VEC) {
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = *reinterpret_cast<const float4*>(src + r[k] * ld + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc.x = fmaf(wj[k], x[k].x, acc.x);
          acc.y = fmaf(wj[k], x[k].y, acc.y);
          acc.z = fmaf(wj[k], x[k].z, acc.z);
          acc.w = fmaf(wj[k], x[k].w, acc.w);
        }
      } else {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = src[r[k] * ld + c];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.x = fmaf(wj[k], x[k], acc.x);
      }
    }
  }
  for (; u < cnt; ++u) {
    const float wj = lane_bcast(wl, u);
    const int64_t r = __builtin_amdgcn_readlane(rl, u);
    if (act) {
      if constexpr (VEC) {
        const float4 x = *reinterpret_cast<const float4*>(src + r * ld + c);
        acc.x = fmaf(wj, x.x, acc.x);
        acc.y = fmaf(wj, x.y, acc.y);
        acc.z = fmaf(wj, x.z, acc.z);
        acc.w = fmaf(wj, x.w, acc.w);
      } else {
        acc.x = fmaf(wj, src[r * ld + c], acc.x);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gat_scores_kernel(const float* __restrict__ h, int64_t ldh, int64_t n_h, int d,
                                                         const float* __restrict__ a,
                                                         const int32_t* __restrict__ rows, int64_t n_rows,
                                                         float* __restrict__ s_l, float* __restrict__ s_r) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_rows) return;
  const int64_t u = rows ? (int64_t)rows[t] : t;
  if ((uint64_t)u >= (uint64_t)n_h) return;
  const float* x = h + u * ldh;
  float l = 0.f, r = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float xv = x[c];
    l = fmaf(a[c], xv, l);
    r = fmaf(a[d + c], xv, r);
  }
  l = wave_sum(l);
  r = wave_sum(r);
  if (lane == 0) {
    s_l[u] = l;
    s_r[u] = r;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gat_forward_kernel(
    const float* __restrict__ h, int64_t ldh, int64_t n_h, int d, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ hrow, const float* __restrict__ cw, const int32_t* __restrict__ own, int64_t n_seg,
    const float* __restrict__ s_l, const float* __restrict__ s_r, float* __restrict__ out, int64_t ldo,
    float* __restrict__ p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_seg) return;
  const int64_t b = seg_ptr[row], e = seg_ptr[row + 1];
  const int32_t ro = own[row];
  const bool own_ok = (uint64_t)(int64_t)ro < (uint64_t)n_h;
  const float sl = own_ok ? s_l[ro] : 0.f;
  float M = -INFINITY;
  for (int64_t j = b + lane; j < e; j += 64) {
    const GatEdge g = gat_edge(sl, own_ok, s_r, hrow[j], n_h, cw[j]);
    if (g.keep) M = fmaxf(M, g.m);
  }
  M = wave_max(M);
  float S = 0.f;
  for (int64_t j = b + lane; j < e; j += 64) {
    const GatEdge g = gat_edge(sl, own_ok, s_r, hrow[j], n_h, cw[j]);
    if (g.keep) S += expf(g.m - M);
  }
  S = wave_sum(S);  // >= 1 once anything is kept (the maximum's own term)
  float* o = out + row * ldo;
  constexpr int kCols = VEC ? 256 : 64;
  for (int c0 = 0; c0 < d; c0 += kCols) {
    const int c = c0 + (VEC ? 4 * lane : lane);
    const bool act = c < d;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t j0 = b; j0 < e; j0 += 64) {
      const int64_t j = j0 + lane;
      float pj = 0.f;
      int32_t rj = 0;
      if (j < e) {
        const int32_t r = hrow[j];
        const GatEdge g = gat_edge(sl, own_ok, s_r, r, n_h, cw[j]);
        if (g.keep) pj = expf(g.m - M) / S;
        if ((uint64_t)(int64_t)r < (uint64_t)n_h) rj = r;
        if (c0 == 0) p[j] = pj;
      }
      const int64_t left = e - j0;
      chunk_gather<VEC>(h, ldh, c, act, pj, rj, left < 64 ? (int)left : 64, acc);
    }
    if (act) {
      if constexpr (VEC)
        *reinterpret_cast<float4*>(o + c) = acc;
      else
        o[c] = acc.x;
    }
  }
}

// lane partial of dout_i . h[r] over this lane's columns, ascending
template <bool VEC>
__device__ __forceinline__ float gat_row_dot(const float* __restrict__ x, const float* __restrict__ y, int d,
                                             int lane) {
  float part = 0.f;
  if constexpr (VEC) {
    for (int c = 4 * lane; c < d; c += 256) {
      const float4 xv = *reinterpret_cast<const float4*>(x + c);
      const float4 yv = *reinterpret_cast<const float4*>(y + c);
      part = fmaf(xv.x, yv.x, part);
      part = fmaf(xv.y, yv.y, part);
      part = fmaf(xv.z, yv.z, part);
      part = fmaf(xv.w, yv.w, part);
    }
  } else {
    for (int c = lane; c < d; c += 64) part = fmaf(x[c], y[c], part);
  }
  return part;
}

template <bool VEC>
__global__ __launch_bounds__(256) void gat_backward_edges_kernel(
    const float* __restrict__ h, int64_t ldh, int64_t n_h, int d, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ hrow, const float* __restrict__ cw, const int32_t* __restrict__ own, int64_t n_seg,
    const float* __restrict__ s_l, const float* __restrict__ s_r, const float* __restrict__ p,
    const float* __restrict__ dout, int64_t lddo, float* __restrict__ de, float* __restrict__ s) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_seg) return;
  const int64_t b = seg_ptr[row], e = seg_ptr[row + 1];
  const int32_t ro = own[row];
  const bool own_ok = (uint64_t)(int64_t)ro < (uint64_t)n_h;
  const float sl = own_ok ? s_l[ro] : 0.f;
  const float* go = dout + row * lddo;
  // pass 1: g_ij into de[j] (entry j0 + u belongs to lane u, here and in pass
  // 2, so a lane reads back only what it stored itself), gbar
  float gbar = 0.f;
  for (int64_t j0 = b; j0 < e; j0 += 64) {
    const int64_t j = j0 + lane;
    float pj = 0.f;
    int32_t rj = 0;
    if (j < e) {
      const int32_t r = hrow[j];
      if ((uint64_t)(int64_t)r < (uint64_t)n_h) {
        rj = r;
        pj = p[j];
      }
    }
    const int64_t left = e - j0;
    const int cnt = left < 64 ? (int)left : 64;
    float g = 0.f;
    int u = 0;
    for (; u + 4 <= cnt; u += 4) {
      float part[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t r = __builtin_amdgcn_readlane(rj, u + k);
        part[k] = gat_row_dot<VEC>(h + r * ldh, go, d, lane);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        part[k] = wave_sum(part[k]);
        if (lane == u + k) g = part[k];
      }
    }
    for (; u < cnt; ++u) {
      const int64_t r = __builtin_amdgcn_readlane(rj, u);
      const float part = wave_sum(gat_row_dot<VEC>(h + r * ldh, go, d, lane));
      if (lane == u) g = part;
    }
    if (j < e) {
      de[j] = g;
      gbar = fmaf(pj, g, gbar);
    }
  }
  gbar = wave_sum(gbar);
  // pass 2
  float ssum = 0.f;
  for (int64_t j = b + lane; j < e; j += 64) {
    const float c = cw[j];
    const GatEdge g = gat_edge(sl, own_ok, s_r, hrow[j], n_h, c);
    const float pj = p[j];
    float v = 0.f;
    if (g.keep && pj != 0.f) v = pj * (de[j] - gbar) * c * (g.e > 0.f ? 1.f : kGatSlope);
    de[j] = v;
    ssum += v;
  }
  ssum = wave_sum(ssum);
  if (lane == 0) s[row] = ssum;
}

template <bool VEC>
__global__ __launch_bounds__(256) void gat_backward_rows_kernel(
    int64_t n_h, int d, const float* __restrict__ a, const int32_t* __restrict__ rows_u, int64_t n_rows,
    const int64_t* __restrict__ segT, const int32_t* __restrict__ entT, const int32_t* __restrict__ segofT,
    const int64_t* __restrict__ own_ptr, const int32_t* __restrict__ own_seg, const float* __restrict__ p,
    const float* __restrict__ de, const float* __restrict__ s, int64_t nnz, int64_t n_seg,
    const float* __restrict__ dout, int64_t lddo, float* __restrict__ dh, int64_t lddh, float* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_rows) return;
  const int64_t u = rows_u[t];
  if ((uint64_t)u >= (uint64_t)n_h) {  // (no such row: nothing to write, and no part in da)
    if (lane == 0) coef[t] = coef[n_rows + t] = 0.f;
    return;
  }
  const int64_t b = segT[t], e = segT[t + 1];
  float cr = 0.f;
  for (int64_t j = b + lane; j < e; j += 64) {
    const int64_t k = entT[j];
    if ((uint64_t)k < (uint64_t)nnz) cr += de[k];
  }
  cr = wave_sum(cr);
  float cl = 0.f;
  for (int64_t j = own_ptr[t] + lane; j < own_ptr[t + 1]; j += 64) {
    const int64_t i = own_seg[j];
    if ((uint64_t)i < (uint64_t)n_seg) cl += s[i];
  }
  cl = wave_sum(cl);
  if (lane == 0) {
    coef[t] = cl;
    coef[n_rows + t] = cr;
  }
  float* o = dh + u * lddh;
  constexpr int kCols = VEC ? 256 : 64;
  for (int c0 = 0; c0 < d; c0 += kCols) {
    const int c = c0 + (VEC ? 4 * lane : lane);
    const bool act = c < d;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t j0 = b; j0 < e; j0 += 64) {
      const int64_t j = j0 + lane;
      float pj = 0.f;
      int32_t rj = 0;
      if (j < e) {
        const int64_t k = entT[j];
        const int32_t i = segofT[j];
        if ((uint64_t)k < (uint64_t)nnz && (uint64_t)(int64_t)i < (uint64_t)n_seg) {
          pj = p[k];
          rj = i;
        }
      }
      const int64_t left = e - j0;
      chunk_gather<VEC>(dout, lddo, c, act, pj, rj, left < 64 ? (int)left : 64, acc);
    }
    if (act) {
      if constexpr (VEC) {
        acc.x = fmaf(cr, a[d + c], fmaf(cl, a[c], acc.x));
        acc.y = fmaf(cr, a[d + c + 1], fmaf(cl, a[c + 1], acc.y));
        acc.z = fmaf(cr, a[d + c + 2], fmaf(cl, a[c + 2], acc.z));
        acc.w = fmaf(cr, a[d + c + 3], fmaf(cl, a[c + 3], acc.w));
        *reinterpret_cast<float4*>(o + c) = acc;
      } else {
        o[c] = fmaf(cr, a[d + c], fmaf(cl, a[c], acc.x));
      }
    }
  }
}

// partial[blk][0..d) = sum_t cl_t h[u_t][c], partial[blk][d..2d) = sum_t cr_t
// h[u_t][c] over the block's kGatDaRows rows in order; one thread per column.
__global__ __launch_bounds__(256) void gat_da_partial_kernel(const float* __restrict__ h, int64_t ldh, int64_t n_h,
                                                             int d, const int32_t* __restrict__ rows_u,
                                                             int64_t n_rows, const float* __restrict__ coef,
                                                             float* __restrict__ partial) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const int64_t t0 = (int64_t)blockIdx.x * kGatDaRows;
  const int64_t t1 = t0 + kGatDaRows < n_rows ? t0 + kGatDaRows : n_rows;
  float l = 0.f, r = 0.f;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t u = rows_u[t];
    if ((uint64_t)u >= (uint64_t)n_h) continue;
    const float x = h[u * ldh + c];
    l = fmaf(coef[t], x, l);
    r = fmaf(coef[n_rows + t], x, r);
  }
  float* o = partial + (int64_t)blockIdx.x * 2 * d;
  o[c] = l;
  o[d + c] = r;
}

__global__ __launch_bounds__(256) void gat_da_reduce_kernel(const float* __restrict__ partial, int64_t n_blk, int d2,
                                                            float* __restrict__ da) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d2) return;
  float v = 0.f;
  for (int64_t k = 0; k < n_blk; ++k) v += partial[k * d2 + c];
  da[c] = v;
}

static bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

void launch_gat_node_scores(const float* h, int64_t ldh, int64_t n_h, int d, const float* a, const int32_t* rows,
                            int64_t n_rows, float* s_l, float* s_r, hipStream_t st) {
  hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, st, h, ldh, n_h, d, a,
                     rows, n_rows, s_l, s_r);
}

void launch_gat_forward(const float* h, int64_t ldh, int64_t n_h, int d, const int64_t* seg_ptr, const int32_t* hrow,
                        const float* c, const int32_t* own, int64_t n_seg, const float* s_l, const float* s_r,
                        float* out, int64_t ldo, float* p, hipStream_t st) {
  const bool vec = d % 4 == 0 && ldh % 4 == 0 && ldo % 4 == 0 && aligned16(h) && aligned16(out);
  const dim3 grid((unsigned)ceil_div(n_seg, 4)), block(256);
  if (vec)
    hipLaunchKernelGGL(gat_forward_kernel<true>, grid, block, 0, st, h, ldh, n_h, d, seg_ptr, hrow, c, own, n_seg,
                       s_l, s_r, out, ldo, p);
  else
    hipLaunchKernelGGL(gat_forward_kernel<false>, grid, block, 0, st, h, ldh, n_h, d, seg_ptr, hrow, c, own, n_seg,
                       s_l, s_r, out, ldo, p);
}

void launch_gat_backward_edges(const float* h, int64_t ldh, int64_t n_h, int d, const int64_t* seg_ptr,
                               const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg,
                               const float* s_l, const float* s_r, const float* p, const float* dout, int64_t lddo,
                               float* de, float* s, hipStream_t st) {
  const bool vec = d % 4 == 0 && ldh % 4 == 0 && lddo % 4 == 0 && aligned16(h) && aligned16(dout);
  const dim3 grid((unsigned)ceil_div(n_seg, 4)), block(256);
  if (vec)
    hipLaunchKernelGGL(gat_backward_edges_kernel<true>, grid, block, 0, st, h, ldh, n_h, d, seg_ptr, hrow, c, own,
                       n_seg, s_l, s_r, p, dout, lddo, de, s);
  else
    hipLaunchKernelGGL(gat_backward_edges_kernel<false>, grid, block, 0, st, h, ldh, n_h, d, seg_ptr, hrow, c, own,
                       n_seg, s_l, s_r, p, dout, lddo, de, s);
}

void launch_gat_backward_rows(const float* h, int64_t ldh, int64_t n_h, int d, const float* a, const int32_t* rows_u,
                              int64_t n_rows, const int64_t* segT, const int32_t* entT, const int32_t* segofT,
                              const int64_t* own_ptr, const int32_t* own_seg, const float* p, const float* de,
                              const float* s, int64_t nnz, int64_t n_seg, const float* dout, int64_t lddo, float* dh,
                              int64_t lddh, float* coef, float* partial, float* da, hipStream_t st) {
  const bool vec = d % 4 == 0 && lddo % 4 == 0 && lddh % 4 == 0 && aligned16(dout) && aligned16(dh);
  const dim3 grid((unsigned)ceil_div(n_rows, 4)), block(256);
  if (vec)
    hipLaunchKernelGGL(gat_backward_rows_kernel<true>, grid, block, 0, st, n_h, d, a, rows_u, n_rows, segT, entT,
                       segofT, own_ptr, own_seg, p, de, s, nnz, n_seg, dout, lddo, dh, lddh, coef);
  else
    hipLaunchKernelGGL(gat_backward_rows_kernel<false>, grid, block, 0, st, n_h, d, a, rows_u, n_rows, segT, entT,
                       segofT, own_ptr, own_seg, p, de, s, nnz, n_seg, dout, lddo, dh, lddh, coef);
  const int n_blk = ceil_div(n_rows, kGatDaRows);
  hipLaunchKernelGGL(gat_da_partial_kernel, dim3((unsigned)n_blk, (unsigned)ceil_div(d, 256)), block, 0, st, h, ldh,
                     n_h, d, rows_u, n_rows, coef, partial);
  hipLaunchKernelGGL(gat_da_reduce_kernel, dim3((unsigned)ceil_div(2 * (int64_t)d, 256)), block, 0, st, partial,
                     (int64_t)n_blk, 2 * d, da);
}

}  // namespace ps

using namespace ps;

extern "C" {

int pinsage_segment_wmean(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                          const int32_t* cols, const float* w, int64_t n_seg, int normalize, float* out,
                          int64_t ldo, void* stream) {
  if (n_seg < 0 || d <= 0 || d > (1 << 24) || n_h < 0 || ldh < d || ldo < d || !seg_ptr ||
      (n_seg > 0 && !out) || (n_h > 0 && !h)) {
    set_error("segment_wmean: bad argument");
    return kErrArg;
  }
  if (n_seg == 0) return kOk;
  const bool vec = n_h > 0 && d % 4 == 0 && ldh % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)h & 15) == 0 &&
                   ((uintptr_t)out & 15) == 0;
  const dim3 grid((unsigned)ceil_div(n_seg, 4)), block(256);
  if (vec)
    hipLaunchKernelGGL(segment_wmean_kernel<true>, grid, block, 0, (hipStream_t)stream, h, ldh, n_h, (int)d,
                       seg_ptr, cols, w, n_seg, normalize, out, ldo);
  else
    hipLaunchKernelGGL(segment_wmean_kernel<false>, grid, block, 0, (hipStream_t)stream, h, ldh, n_h, (int)d,
                       seg_ptr, cols, w, n_seg, normalize, out, ldo);
  PS_CHECK_LAUNCH();
  return kOk;
}

// d, n_h and the leading dimension of h shared by every pinsage_gat_* entry
static bool gat_dims_ok(int64_t ldh, int64_t n_h, int64_t d) {
  return d > 0 && d <= (1 << 20) && n_h >= 0 && n_h <= INT32_MAX && ldh >= d;
}

int64_t pinsage_gat_partial_rows(int64_t n_rows) {
  if (n_rows < 0 || n_rows > INT32_MAX) {
    set_error("gat_partial_rows: bad argument");
    return kErrArg;
  }
  return ceil_div(n_rows, kGatDaRows);
}

int pinsage_gat_node_scores(const float* h, int64_t ldh, int64_t n_h, int64_t d, const float* a, const int32_t* rows,
                            int64_t n_rows, float* s_l, float* s_r, void* stream) {
  if (!gat_dims_ok(ldh, n_h, d) || !a || n_rows < 0 || n_rows > INT32_MAX || (!rows && n_rows > n_h) ||
      (n_rows > 0 && n_h > 0 && (!h || !s_l || !s_r))) {
    set_error("gat_node_scores: bad argument");
    return kErrArg;
  }
  if (n_rows == 0 || n_h == 0) return kOk;
  launch_gat_node_scores(h, ldh, n_h, (int)d, a, rows, n_rows, s_l, s_r, (hipStream_t)stream);
  PS_CHECK_LAUNCH();
  return kOk;
}

int pinsage_gat_forward(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                        const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg, int64_t nnz,
                        const float* s_l, const float* s_r, float* out, int64_t ldo, float* p, void* stream) {
  if (!gat_dims_ok(ldh, n_h, d) || n_seg < 0 || n_seg > INT32_MAX || nnz < 0 || ldo < d || !seg_ptr ||
      (n_seg > 0 && (!out || !own)) || (nnz > 0 && (!hrow || !c || !p)) || (n_h > 0 && (!h || !s_l || !s_r))) {
    set_error("gat_forward: bad argument");
    return kErrArg;
  }
  if (n_seg == 0) return kOk;
  if (n_h == 0) {  // no row to attend to: every segment is empty of kept entries
    PS_CHECK_HIP(hipMemset2DAsync(out, ldo * sizeof(float), 0, d * sizeof(float), n_seg, (hipStream_t)stream));
    if (nnz > 0) PS_CHECK_HIP(hipMemsetAsync(p, 0, nnz * sizeof(float), (hipStream_t)stream));
    return kOk;
  }
  launch_gat_forward(h, ldh, n_h, (int)d, seg_ptr, hrow, c, own, n_seg, s_l, s_r, out, ldo, p, (hipStream_t)stream);
  PS_CHECK_LAUNCH();
  return kOk;
}

int pinsage_gat_backward_edges(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                               const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg, int64_t nnz,
                               const float* s_l, const float* s_r, const float* p, const float* dout, int64_t lddo,
                               float* de, float* s, void* stream) {
  if (!gat_dims_ok(ldh, n_h, d) || n_seg < 0 || n_seg > INT32_MAX || nnz < 0 || lddo < d || !seg_ptr ||
      (n_seg > 0 && (!dout || !own || !s)) || (nnz > 0 && (!hrow || !c || !p || !de)) ||
      (n_h > 0 && (!h || !s_l || !s_r))) {
    set_error("gat_backward_edges: bad argument");
    return kErrArg;
  }
  if (n_seg == 0) return kOk;
  if (n_h == 0) {
    PS_CHECK_HIP(hipMemsetAsync(s, 0, n_seg * sizeof(float), (hipStream_t)stream));
    if (nnz > 0) PS_CHECK_HIP(hipMemsetAsync(de, 0, nnz * sizeof(float), (hipStream_t)stream));
    return kOk;
  }
  launch_gat_backward_edges(h, ldh, n_h, (int)d, seg_ptr, hrow, c, own, n_seg, s_l, s_r, p, dout, lddo, de, s,
                            (hipStream_t)stream);
  PS_CHECK_LAUNCH();
  return kOk;
}

int pinsage_gat_backward_rows(const float* h, int64_t ldh, int64_t n_h, int64_t d, const float* a,
                              const int32_t* rows_u, int64_t n_rows, const int64_t* segT, const int32_t* entT,
                              const int32_t* segofT, const int64_t* own_ptr, const int32_t* own_seg, const float* p,
                              const float* de, const float* s, int64_t nnz, int64_t n_seg, const float* dout,
                              int64_t lddo, float* dh, int64_t lddh, float* coef, float* partial, float* da,
                              void* stream) {
  if (!gat_dims_ok(ldh, n_h, d) || !a || !da || n_rows < 0 || n_rows > n_h || nnz < 0 || n_seg < 0 ||
      n_seg > INT32_MAX || lddo < d || lddh < d ||
      (n_rows > 0 && (!h || !rows_u || !segT || !own_ptr || !dh || !coef || !partial)) ||
      (nnz > 0 && n_rows > 0 && (!entT || !segofT || !p || !de)) ||
      (n_seg > 0 && n_rows > 0 && (!own_seg || !s || !dout))) {
    set_error("gat_backward_rows: bad argument");
    return kErrArg;
  }
  if (n_rows == 0) {
    PS_CHECK_HIP(hipMemsetAsync(da, 0, 2 * d * sizeof(float), (hipStream_t)stream));
    return kOk;
  }
  launch_gat_backward_rows(h, ldh, n_h, (int)d, a, rows_u, n_rows, segT, entT, segofT, own_ptr, own_seg, p, de, s,
                           nnz, n_seg, dout, lddo, dh, lddh, coef, partial, da, (hipStream_t)stream);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // extern "C"
