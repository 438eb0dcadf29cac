// On-the-fly sampling of a train step's model calls on the device (fly.hip);
// the arguments are those of the pinsage_fly_* entry points (pinsage_hip.h).
#pragma once
#include "common.h"

namespace ps {

int64_t fly_workspace_bytes(int64_t n, int64_t B, int64_t L, int64_t T, int64_t n_hops);
int fly_init_workspace(void* ws, int64_t n, int64_t B, int64_t L, int64_t T, int64_t n_hops, hipStream_t st);

// err[0..1] into the host ring slot (*ctr % R) at byte err_off
int fly_publish_err(const int* err, void* ring, int64_t slot_bytes, int64_t R, const int64_t* ctr, int64_t err_off,
                    hipStream_t st);

// zero the step's Adam coefficient coef[1] when its sampling failed (err)
int fly_gate_adam(int* err, float* coef, hipStream_t st);

int fly_sample(const int64_t* indptr, const int32_t* indices, int64_t n_all, const int64_t* batch, int64_t B,
               int64_t n, int64_t L, int64_t T, int64_t n_hops, float alpha, const uint64_t* seeds, void* ws,
               int64_t ws_bytes, int32_t* const* nbt_host, float* const* wnt_host, int32_t** tab_ptrs_dev,
               int64_t rows_cap, int64_t* pos_ids, int* n_x, int64_t* ids_xo, int64_t x_cap, const float* feats,
               int64_t ld_f, int64_t d, float* fx, int64_t ld_x, int* err, hipStream_t st);

}  // namespace ps
