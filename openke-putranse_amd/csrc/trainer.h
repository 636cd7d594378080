// What capi.cpp, legacy.cpp and the trainer runtime (trainer.cpp) share: the sampler object and the model descriptor check.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "graph.h"
#include "kernels.h"

struct pt_sampler {
    pt::Graph *g = nullptr;        // graph sampled from (follows swaps for the legacy context)
    int64_t threads = 0;
    uint64_t *d_states = nullptr;  // device LCG states, one per emulated sampler thread
    int device = -1;
    ~pt_sampler() {
        if (d_states) (void)hipFree(d_states);
    }
};

namespace pt {

// binds `s` to `g` (uploaded; null: bound later) with `threads` device streams seeded from `seeds` (null: zeros)
int sampler_init(pt_sampler *s, Graph *g, int64_t threads, const uint64_t *seeds);
// checks a model descriptor and fills the kernels' parameters from it
int desc_to_params(const pt_model_desc *m, StepParams &P);

}  // namespace pt
