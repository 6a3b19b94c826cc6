// nco_device.h -- the Mixer's per-sample arithmetic (mixers.h:169-188), shared
// by the mixer kernels (mixer.hip) and the interpolator -> mixer epilogue
// (upmix.hip).
#pragma once
#include "common.h"

namespace srcdsp {

__device__ __forceinline__ uint32_t nco_mix(uint32_t w, const int16_t *tab, unsigned N, unsigned phi) {
    unsigned ic = phi + N / 4;  // (phi + N/4) % N, phi < N
    ic = ic >= N ? ic - N : ic;
    const int32_t lr = tab[ic], li = tab[phi];
    const int32_t ar = sext16(w), ai = sext16_hi(w);
    // ::operator*(complex<int16_t>, complex<int32_t>) (dsp_complex.cpp:31-37); |T| <= 16383 so no wrap
    const int32_t r = ar * lr - ai * li;
    const int32_t i = ai * lr + li * ar;
    return pack16(limit16(r, 14), limit16(i, 14));
}

__device__ __forceinline__ unsigned phase_at(unsigned long idx, unsigned phi0, unsigned freq, unsigned N) {
    return (unsigned)(((unsigned long)phi0 + (idx % N) * (unsigned long)freq) % N);
}

}  // namespace srcdsp
