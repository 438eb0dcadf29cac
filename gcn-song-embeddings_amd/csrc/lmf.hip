// Logistic matrix factorisation, full-gradient AdaGrad ascent (definition: lmf.h).
//
// The dense term D = sigmoid(X Y^T + bx + by^T) Y and its row sums: the BIAS form
// of sig_dense_kernel (sig_dense.h), which describes the kernel.
//
// The sparse part and the AdaGrad step: the BIAS form of sig_update_kernel
// (sig_update.h), which describes the kernel.
#include <algorithm>
#include <cmath>

#include "lmf.h"
#include "sig_update.h"

namespace ps {

int lmf_row_block() { return kSigRowBlock; }
int lmf_long_row() { return kRowLong; }

int launch_lmf_dense(const float* X, const float* bx, int64_t n_rows, int64_t ldx, const float* Y, const float* by,
                     int64_t n_other, int64_t ldy, int64_t f, float* D, int64_t ldd, float* dsum, hipStream_t st) {
  PS_TRY(row_tables_ok("lmf_dense", f, {{"X", X, ldx}, {"Y", Y, ldy}, {"D", D, ldd}}));
  PS_REQUIRE(bx != nullptr && by != nullptr && dsum != nullptr, kErrArg, "lmf_dense: null bias or dsum");
  PS_TRY(row_sizes_ok("lmf_dense", n_rows, n_other));
  if (n_rows == 0) return kOk;
  sig_dense_launch<false>(SigDenseArgs{X, bx, n_rows, ldx, Y, by, n_other, ldy, (int)f, D, ldd, dsum}, st);
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
  const SigUpdateArgs A{ptr, n_rows, {idx, val, alpha, Y, by, n_other, ldy, err}, X, bx, ldx, (int)f, D, ldd, dsum,
                        nullptr, H, ldh, hb, reg, lr};
  sig_update_launch<false>(A, st);
  PS_CHECK_LAUNCH();
  return kOk;
}

}  // namespace ps
