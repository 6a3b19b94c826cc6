// upmix_kernels.h -- what the interpolator -> mixer kernel (upmix.hip) and the
// mapper -> interpolator -> mixer kernel (modulate.hip) share: the launch
// description, the mixer epilogue of the tile and the shapes the tile takes.
#pragma once
#include "ops.h"

#include "nco_device.h"
#include "up_dot2_kernels.h"

namespace srcdsp {

constexpr unsigned kUpmixMaxN = 4096;  // table entries staged in LDS (8 KiB)

struct UpmixLaunch {
    const uint32_t *in;
    uint32_t *out;
    const uint32_t *pairs;   // shared by all channels
    const int16_t *table;    // one table for all: built from N alone (mixers.h:155-158)
    long n_in, n_total;
    long in_stride, out_stride;  // samples, between channels (grid.y)
    int H;
    unsigned shift, N;
    unsigned tab_off;        // byte offset of the table in dynamic LDS
    const uint32_t *hist_in[kMaxBatch];
    uint32_t *hist_out[kMaxBatch];
    uint32_t mix[kMaxBatch];  // lo: phase, hi: frequency word
};

// the mixer on a lane's consecutive output words
struct UpMixEpilogue {
    const int16_t *tab;
    unsigned N, freq, phi_tile;  // phi_tile: phase of the tile's first output
    unsigned ph;
    __device__ __forceinline__ void begin(int k) { ph = (phi_tile + ((unsigned)k % N) * freq) % N; }
    __device__ __forceinline__ uint32_t operator()(uint32_t w) {
        const uint32_t y = nco_mix(w, tab, N, ph);
        ph += freq;
        ph = ph >= N ? ph - N : ph;
        return y;
    }
};

// the shapes the fused tile takes (d_in: the tile's input buffer)
inline bool upmix_fused_takes(const srcdsp_up_state &u, const MixerState &m, const void *d_in, const void *d_out) {
    return u.variant == UV_CI16_I32 && u.coef_i16 && u.L >= 2 && u.L <= 8 && u.ntaps <= kUpMaxTaps &&
           m.N <= kUpmixMaxN && aligned16(d_in) && aligned16(d_out);
}

}  // namespace srcdsp
