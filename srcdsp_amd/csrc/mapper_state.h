// mapper_state.h -- the symbol mapper's handle and its launcher, shared by
// mapper.hip (srcdsp_mapper_*) and modulate.hip (the mapper ahead of the
// interpolator -> mixer tile).
#pragma once
#include "ops.h"

#include "mapper_kernels.h"

namespace srcdsp {

// A host object until it steps on the device (create makes no device call).
// The state then lives in a device word, because it depends on device-resident
// bits: a step reads d_state[cur] (or, while the host copy is the current one,
// takes it as a launch argument) and writes d_state[cur ^ 1].
struct MapperState {
    int kind = MAPPER_SDPSK;
    int state = 0;                  // the host copy: current unless on_dev
    bool on_dev = false;            // the last step left the state in d_state[cur]
    uint32_t *d_state = nullptr;    // two words, made at the first device step
    int cur = 0;
    GrowBuf par{GrowBuf::kDevice};  // per-tile parities of the calls this handle led
    GrowBuf sym{GrowBuf::kDevice};  // srcdsp_modulate_*: packed SDPSK states, or the chain path's symbols
    GrowBuf rows{GrowBuf::kDevice}; // srcdsp_modulate_sum_step: the carrier rows of the calls this handle led (bank path)
    Ordering order;
    HostStage stage;                // srcdsp_mapper_step_host

    int touch();                    // the device word and the event, once
    int fetch();                    // waits for the last step; the state back on the host
};

// what the kernels get of one channel's state
struct MapperRowState {
    const uint32_t *in;  // read when host < 0
    uint32_t *out;
    int host;
};
// chan_begin / chan_commit of a mapper: the stream waits for the handle's last
// step and the row is named; once the launch is enqueued the written word
// becomes current and the step is recorded
int mapper_begin(MapperState &m, hipStream_t s, MapperRowState &row);
int mapper_commit(MapperState &m, hipStream_t s);

enum MapperOut {
    kMapperSymbols = 0,  // packed complex<int16_t> words, out_stride in words
    kMapperStates = 1,   // SDPSK states, 2 bits each, 16 per word in bit order; out_stride in words
};
// nc <= kMaxBatch mappers of one kind over n_bits > 0 each, checked by the
// caller; `lead` owns the tile-parity scratch
int mapper_launch(MapperState &lead, const srcdsp_mapper_t *hs, int nc, const void *d_bits, size_t bits_stride,
                  void *d_out, size_t out_stride, size_t n_bits, MapperOut mode, hipStream_t s);

}  // namespace srcdsp

struct srcdsp_mapper { srcdsp::MapperState m; };
