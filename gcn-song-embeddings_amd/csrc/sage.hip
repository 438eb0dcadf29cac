// Unsupervised GraphSAGE: the neighbour sample, the negatives and the margin
// loss (definition: sage.h).
//
// sage_neighbours_kernel: one 32-lane half of a wave per node.  The S Philox
// draws of Floyd's algorithm do not depend on one another, so lane j makes draw
// j; only the collision rule is serial, and it is S steps of one cross-lane read
// and one ballot.  The weights' sum is S cross-lane reads in slot order.
//
// sage_negatives_kernel: one lane per sample, as bpr_sample_kernel's draw.
//
// sage_margin_kernel: one wave per anchor group.  Every row of the group is read
// once for its cosine (four rows' loads in flight), the two chosen rows once
// more for the gradient; every lane holds the same wave sums, so the selection
// is the same scalar loop in every lane and nothing is broadcast.
#include <cmath>

#include "philox.h"
#include "sage.h"
#include "sig_dense.h"

namespace ps {

constexpr int kSageBlock = 256;
constexpr int kSageWaves = kSageBlock / 64;  // anchor groups per workgroup of the loss
constexpr int kSageInFlight = 4;             // rows of Z whose loads are in flight per step

struct SageNbArgs {
  const int64_t* ptr;
  const int32_t* idx;
  const int64_t* weight;
  int64_t n_nodes;
  const int64_t* nodes;
  int64_t m;
  int S;
  uint64_t seed;
  uint32_t round64, offset;  // round64 = round * 64: draw j is counter word round64 + j
  int32_t* nb;
  float* w;
  int* err;
};

// no lane leaves early: the cross-lane reads below are the whole wave's
__global__ __launch_bounds__(kSageBlock) void sage_neighbours_kernel(SageNbArgs A) {
  const int tid = threadIdx.x, j = tid & 31, base = tid & 32;
  const int64_t i = ((int64_t)blockIdx.x * kSageBlock + tid) >> 5;
  const bool live = i < A.m;
  const int S = A.S;
  int64_t v = 0, b = 0, deg = 0;
  if (live) {
    v = A.nodes[i];
    if (v < 0 || v >= A.n_nodes) {  // callers validate; clamp so that no access strays
      if (A.err) atomicExch(A.err, 1);
      v = 0;
    }
    b = A.ptr[v];
    deg = A.ptr[v + 1] - b;
    if (deg < 0 || deg > INT32_MAX) {
      if (A.err) atomicExch(A.err, 1);
      deg = 0;
    }
  }
  const bool floyd = deg > S;
  int32_t t = 0, mj = 0, c = j;
  if (floyd && j < S) {
    mj = (int32_t)(deg - S + j + 1);
    const uint4 r = philox10(A.seed, make_uint4(A.round64 + (uint32_t)j, (uint32_t)v, (uint32_t)((uint64_t)v >> 32),
                                                A.offset));
    t = (int32_t)__umul64hi((uint64_t)r.x | ((uint64_t)r.y << 32), (uint64_t)mj);  // < mj
    c = t;
  }
  for (int s = 1; s < S; ++s) {  // lanes below s hold their final c
    const int32_t ts = __shfl(t, base + s, 64);
    const uint64_t hits = __ballot(floyd && j < s && c == ts);
    if (floyd && j == s && (uint32_t)(hits >> base) != 0u) c = mj - 1;
  }
  const bool valid = live && j < S && (floyd || j < deg);
  int32_t nbr = -1;
  float a = 0.f;
  if (valid) {
    const int64_t e = b + c;
    nbr = A.idx[e];
    if (nbr < 0 || nbr >= A.n_nodes) {
      if (A.err) atomicExch(A.err, 1);
      nbr = 0;
    }
    a = A.weight ? sqrtf((float)A.weight[e]) : 1.f;
  }
  float tot = 0.f;
  for (int s = 0; s < S; ++s) tot += __shfl(a, base + s, 64);
  if (live && j < S) {
    A.nb[i * S + j] = nbr;
    A.w[i * S + j] = valid ? a / tot : 0.f;
  }
}

int launch_sage_neighbours(const int64_t* ptr, const int32_t* idx, const int64_t* weight, int64_t n_nodes,
                           const int64_t* nodes, int64_t m, int64_t S, uint64_t seed, int64_t round, uint32_t offset,
                           int32_t* nb, float* w, int* err, hipStream_t st) {
  PS_REQUIRE(S >= 1 && S <= kSageMaxFanout, kErrArg, "sage_neighbours: need 1 <= fanout <= 32");
  PS_REQUIRE(round >= 0 && round < (1 << 25), kErrArg, "sage_neighbours: need 0 <= round < 2^25");
  PS_REQUIRE(n_nodes >= 1 && n_nodes <= INT32_MAX && m >= 0 && m <= INT32_MAX, kErrArg,
             "sage_neighbours: bad sizes");
  PS_REQUIRE(ptr != nullptr && idx != nullptr, kErrArg, "sage_neighbours: null graph");
  if (m == 0) return kOk;
  PS_REQUIRE(nodes != nullptr && nb != nullptr && w != nullptr, kErrArg, "sage_neighbours: null nodes, nb or w");
  const SageNbArgs A{ptr, idx, weight, n_nodes, nodes, m, (int)S, seed, (uint32_t)round * 64u, offset, nb, w, err};
  hipLaunchKernelGGL(sage_neighbours_kernel, dim3((unsigned)ceil_div(m * 32, kSageBlock)), dim3(kSageBlock), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

struct SageNegArgs {
  const int64_t* ptr;
  const int32_t* idx;
  int64_t n_nodes;
  const int64_t* anchors;
  int64_t B;
  int Q;
  uint64_t seed;
  uint32_t round16, offset;  // round16 = round * 16: try k is counter word round16 + k
  int32_t* neg;
  int* err;
};

__global__ __launch_bounds__(kSageBlock) void sage_negatives_kernel(SageNegArgs A) {
  const int64_t o = (int64_t)blockIdx.x * kSageBlock + threadIdx.x;
  if (o >= A.B * A.Q) return;
  int64_t a = A.anchors[o / A.Q];
  if (a < 0 || a >= A.n_nodes) {  // callers validate; clamp so that no access strays
    if (A.err) atomicExch(A.err, 1);
    a = 0;
  }
  const int64_t b = A.ptr[a], e = A.ptr[a + 1];
  const uint64_t t = (uint64_t)(a * A.Q + o % A.Q);
  int32_t jn = -1;
  for (int k = 0; k < kSageTries; ++k) {
    const uint4 r = philox10(A.seed, make_uint4(A.round16 + (uint32_t)k, (uint32_t)t, (uint32_t)(t >> 32), A.offset));
    const int32_t cand = (int32_t)__umulhi(r.x, (uint32_t)A.n_nodes);  // < n_nodes
    if (cand != a && !row_holds(A.idx, b, e, cand)) {
      jn = cand;
      break;
    }
  }
  A.neg[o] = jn;
}

int launch_sage_negatives(const int64_t* ptr, const int32_t* idx, int64_t n_nodes, const int64_t* anchors, int64_t B,
                          int64_t Q, uint64_t seed, int64_t round, uint32_t offset, int32_t* neg, int* err,
                          hipStream_t st) {
  PS_REQUIRE(Q >= 1 && Q <= kSageMaxNeg, kErrArg, "sage_negatives: need 1 <= negatives <= 16");
  PS_REQUIRE(round >= 0 && round < (1 << 27), kErrArg, "sage_negatives: need 0 <= round < 2^27");
  PS_REQUIRE(n_nodes >= 1 && n_nodes <= INT32_MAX && B >= 0 && B <= INT32_MAX, kErrArg, "sage_negatives: bad sizes");
  PS_REQUIRE(ptr != nullptr && idx != nullptr, kErrArg, "sage_negatives: null graph");
  if (B == 0) return kOk;
  PS_REQUIRE(anchors != nullptr && neg != nullptr, kErrArg, "sage_negatives: null anchors or neg");
  const SageNegArgs A{ptr, idx, n_nodes, anchors, B, (int)Q, seed, (uint32_t)round * 16u, offset, neg, err};
  hipLaunchKernelGGL(sage_negatives_kernel, dim3((unsigned)ceil_div(B * Q, kSageBlock)), dim3(kSageBlock), 0, st, A);
  PS_CHECK_LAUNCH();
  return kOk;
}

struct SageLossArgs {
  const float* Z;
  int64_t ldz;
  int d;
  const int32_t* slots;
  int64_t B;
  int P, Q;
  float margin;
  const float* scale;
  float* loss;
  int32_t* active;
  int32_t* sel;
  float* dZ;
  int64_t lddz;
};

// NC = ceil(d / 128): the pairs of columns a lane holds
template <int NC>
__global__ __launch_bounds__(kSageBlock) void sage_margin_kernel(SageLossArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t a = (int64_t)blockIdx.x * kSageWaves + (threadIdx.x >> 6);
  if (a >= A.B) return;  // the whole wave
  const int P = A.P, G = 1 + A.P + A.Q;
  const float* Zg = A.Z + a * G * A.ldz;
  float* dZg = A.dZ + a * G * A.lddz;
  const int32_t* sl = A.slots + a * G;
  bool on[NC];
  int col[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    on[c] = 2 * lane + 128 * c < A.d;
    col[c] = on[c] ? 2 * lane + 128 * c : 0;
  }
  auto load = [&](int g, float2(&y)[NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = row_ld2(Zg + (int64_t)g * A.ldz + col[c], on[c]);
  };
  auto dot = [&](const float2(&x)[NC], const float2(&y)[NC]) __attribute__((always_inline)) {
    float p = fmaf(x[0].x, y[0].x, x[0].y * y[0].y);
#pragma unroll
    for (int c = 1; c < NC; ++c) p = fmaf(x[c].x, y[c].x, fmaf(x[c].y, y[c].y, p));
    return wave_sum(p);
  };
  float2 za[NC];
  load(0, za);
  const float na = dot(za, za);
  // the chosen positive (p) and negative (n): slot, cosine, clamped denominator, squared norm
  int ps = -1, ns = -1;
  float cp = 0.f, cn = 0.f, denp = 1.f, denn = 1.f, nxp = 1.f, nxn = 1.f;
  for (int g0 = 1; g0 < G; g0 += kSageInFlight) {
    float2 y[kSageInFlight][NC];
#pragma unroll
    for (int u = 0; u < kSageInFlight; ++u) load(min(g0 + u, G - 1), y[u]);
#pragma unroll
    for (int u = 0; u < kSageInFlight; ++u) {
      const int g = g0 + u;
      if (g >= G) break;  // wave-uniform
      const float s = dot(za, y[u]), nx = dot(y[u], y[u]);
      if (sl[g] < 0) continue;  // void
      const float den = fmaxf(sqrtf(na * nx), 1e-8f), c = s / den;
      if (g <= P ? (ps < 0 || c < cp) : (ns < 0 || c > cn)) {
        if (g <= P) ps = g, cp = c, denp = den, nxp = nx;
        else ns = g, cn = c, denn = den, nxn = nx;
      }
    }
  }
  const bool act = sl[0] >= 0 && ps >= 0 && ns >= 0;
  const float l = act ? (lmf_softplus(-cp) - lmf_softplus(-cn)) + A.margin : 0.f;
  const bool hinge = act && l > 0.f;
  if (lane == 0) {
    A.loss[a] = hinge ? l : 0.f;
    A.active[a] = act ? 1 : 0;
    A.sel[2 * a] = ps;
    A.sel[2 * a + 1] = ns;
  }
  float2 da[NC], dp[NC], dn[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) da[c] = dp[c] = dn[c] = make_float2(0.f, 0.f);
  if (hinge) {  // wave-uniform
    const float sc = *A.scale;
    const float gp = -lmf_sigmoid(-cp) * sc, gn = lmf_sigmoid(-cn) * sc;  // d loss / d c_pos, d c_neg
    // c = s / den: d c / d z_a = z_x / den - (c / |z_a|^2) z_a, the second term absent under the clamp
    const float kp = gp / denp, kn = gn / denn;
    const float ap = denp > 1e-8f ? gp * cp / na : 0.f, an = denn > 1e-8f ? gn * cn / na : 0.f;
    const float xp = denp > 1e-8f ? gp * cp / nxp : 0.f, xn = denn > 1e-8f ? gn * cn / nxn : 0.f;
    float2 zp[NC], zn[NC];
    load(ps, zp);
    load(ns, zn);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      da[c].x = (kp * zp[c].x - ap * za[c].x) + (kn * zn[c].x - an * za[c].x);
      da[c].y = (kp * zp[c].y - ap * za[c].y) + (kn * zn[c].y - an * za[c].y);
      dp[c].x = kp * za[c].x - xp * zp[c].x;
      dp[c].y = kp * za[c].y - xp * zp[c].y;
      dn[c].x = kn * za[c].x - xn * zn[c].x;
      dn[c].y = kn * za[c].y - xn * zn[c].y;
    }
  }
  for (int g = 0; g < G; ++g) {
    const bool isa = hinge && g == 0, isp = hinge && g == ps, isn = hinge && g == ns;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (on[c])
        *reinterpret_cast<float2*>(dZg + (int64_t)g * A.lddz + col[c]) =
            isa ? da[c] : (isp ? dp[c] : (isn ? dn[c] : make_float2(0.f, 0.f)));
  }
}

int launch_sage_margin_loss(const float* Z, int64_t ldz, int64_t d, const int32_t* slots, int64_t B, int64_t P,
                            int64_t Q, float margin, const float* scale, float* loss, int32_t* active, int32_t* sel,
                            float* dZ, int64_t lddz, hipStream_t st) {
  PS_REQUIRE(d >= 4 && d <= kSageMaxD && d % 4 == 0, kErrArg, "sage_margin_loss: need 4 <= d <= 512, d % 4 == 0");
  PS_REQUIRE(ldz >= d && ldz % 4 == 0 && lddz >= d && lddz % 4 == 0, kErrArg,
             "sage_margin_loss: leading dimensions must be >= d and multiples of 4");
  PS_REQUIRE(P >= 1 && P <= kSageMaxPos && Q >= 1 && Q <= kSageMaxNeg, kErrArg,
             "sage_margin_loss: need 1 <= P <= 64, 1 <= Q <= 16");
  PS_REQUIRE(margin > -INFINITY && margin < INFINITY, kErrArg, "sage_margin_loss: margin must be finite");
  PS_REQUIRE(B >= 0 && B * (1 + P + Q) <= INT32_MAX, kErrArg, "sage_margin_loss: bad sizes");
  if (B == 0) return kOk;
  PS_REQUIRE(Z && slots && scale && loss && active && sel && dZ, kErrArg, "sage_margin_loss: null pointer");
  PS_REQUIRE(((uintptr_t)Z & 15) == 0 && ((uintptr_t)dZ & 15) == 0, kErrArg,
             "sage_margin_loss: Z and dZ must be 16-byte aligned");
  const SageLossArgs A{Z, ldz, (int)d, slots, B, (int)P, (int)Q, margin, scale, loss, active, sel, dZ, lddz};
  const dim3 grid((unsigned)ceil_div(B, kSageWaves)), block(kSageBlock);
  switch (ceil_div(d, 128)) {
    case 1: hipLaunchKernelGGL(sage_margin_kernel<1>, grid, block, 0, st, A); break;
    case 2: hipLaunchKernelGGL(sage_margin_kernel<2>, grid, block, 0, st, A); break;
    case 3: hipLaunchKernelGGL(sage_margin_kernel<3>, grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL(sage_margin_kernel<4>, grid, block, 0, st, A); break;
  }
  PS_CHECK_LAUNCH();
  return kOk;
}

__global__ __launch_bounds__(kSageBlock) void sage_lrelu_backward_kernel(const float* __restrict__ y, int64_t ldy,
                                                                         const float* dy, int64_t lddy, int64_t n,
                                                                         int d4, float* dp, int64_t ldp) {
  const int64_t total = n * d4;
  for (int64_t q = (int64_t)blockIdx.x * kSageBlock + threadIdx.x; q < total; q += (int64_t)gridDim.x * kSageBlock) {
    const int64_t i = q / d4;
    const int c = 4 * (int)(q % d4);
    const float4 yy = *reinterpret_cast<const float4*>(y + i * ldy + c);
    const float4 g = *reinterpret_cast<const float4*>(dy + i * lddy + c);
    *reinterpret_cast<float4*>(dp + i * ldp + c) =
        make_float4(g.x * lrelu_grad(yy.x), g.y * lrelu_grad(yy.y), g.z * lrelu_grad(yy.z), g.w * lrelu_grad(yy.w));
  }
}

int launch_sage_lrelu_backward(const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t n, int64_t d,
                               float* dp, int64_t ldp, hipStream_t st) {
  PS_REQUIRE(n >= 0 && d >= 4 && d % 4 == 0 && d <= (1 << 20) && n * d <= ((int64_t)1 << 40), kErrArg,
             "sage_lrelu_backward: bad sizes");
  if (n == 0) return kOk;
  PS_REQUIRE(row_table_ok(y, d, ldy) && row_table_ok(dy, d, lddy) && row_table_ok(dp, d, ldp), kErrArg,
             "sage_lrelu_backward: tables must be 16-byte aligned with ld >= d, ld % 4 == 0");
  hipLaunchKernelGGL(sage_lrelu_backward_kernel, dim3((unsigned)grid_for(n * (d / 4), kSageBlock)), dim3(kSageBlock), 0,
                     st, y, ldy, dy, lddy, n, (int)(d / 4), dp, ldp);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
