// Host helpers of capi.hip that the batch sampler runtime (loader.hip) shares.
#pragma once
#include "common.h"
#include "mt19937.h"

namespace ps {

// sample_batch with easy negatives (pinsage_training.py:53-77, 89-97)
int sample_batch_easy(MTState& g, const int64_t* positives, int64_t P, int64_t n_items, int64_t batch_size,
                      int64_t* batch_out, int64_t* nodeset_out, int64_t* n_nodeset);

}  // namespace ps
