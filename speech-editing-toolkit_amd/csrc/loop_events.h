// The events of one set_diffusion_loop call (layer spans, loop time, fork and joins of the utterance groups): whatever path the call
// returns by, every event created here is destroyed.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

struct LoopEvents {
    std::vector<hipEvent_t> owned;
    ~LoopEvents() {  // (the one holder of a call is never copied)
        for (hipEvent_t e : owned) (void)hipEventDestroy(e);
    }
    // a new event in *e (timing: one that hipEventElapsedTime can read), owned by the holder
    hipError_t create(hipEvent_t *e, bool timing) {
        const hipError_t rc = timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
        if (rc == hipSuccess) owned.push_back(*e);
        return rc;
    }
};
