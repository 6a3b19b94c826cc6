// stagger_state.h -- the Q-rail stagger's handle, shared by stagger.hip
// (srcdsp_stagger_*) and modulate_offset.hip (the stagger inside the
// mapper -> interpolator -> mixer tile).
#pragma once
#include "ops.h"

#include "stagger_kernels.h"

namespace srcdsp {

// A host object until it steps on the device (create makes no device call).
// The carry then lives in d_hist[cur], double-buffered and ordered like the
// interpolator's history: a step reads d_hist[cur] and writes d_hist[cur ^ 1].
struct StaggerState {
    unsigned D = 1;
    int16_t h_carry[kStaggerMaxD] = {};  // the host copy: current unless on_dev
    bool on_dev = false;                 // the last step left the carry in d_hist[cur]
    void *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    GrowBuf scratch{GrowBuf::kDevice};   // srcdsp_modulate_offset_*: the interpolator's output on the sequence path
    Ordering order;
    HostStage stage;                     // srcdsp_stagger_step_host

    int touch();  // the device buffers and the event, once
    int fetch();  // waits for the last step; the carry back on the host
};

// chan_begin / chan_commit of a stagger: the stream waits for the handle's
// last step, a carry the host holds is sent to d_hist[cur], and the buffers
// the step reads and writes are named; once the launch is enqueued the written
// one becomes current and the step is recorded
int stagger_begin(StaggerState &g, hipStream_t s, const int16_t *&in, int16_t *&out);
int stagger_commit(StaggerState &g, hipStream_t s);

}  // namespace srcdsp

struct srcdsp_stagger { srcdsp::StaggerState g; };
