// corr_all_walk.h -- the in-order walk behind srcdsp_corr_step_all, written
// once for host and device: the resolve kernel (corr_all.hip) and the host
// program tests/cpp/corr_all_host.cpp compile this one source.
//
// The call is the loop of FixedPatternCorrelator::step on the remainders
// (correlators.h:209-303).  step breaks at a detection before `top` advances
// (:291-296), so the next call overwrites the detected sample in the ring: the
// loop scans the stream with every detected sample deleted.  With det[] the
// detected samples so far, the registers after processing sample j are the
// direct sums over j and the N - 1 samples before it that are not in det[]
// (S == 1).  A deletion at q changes those sums for j = q + 1 .. q + N - 1
// only, and the three-register peak test for j = q + 1 .. q + N + 1; outside
// these patches the test is the one of the undisturbed stream, which the
// candidate pass has evaluated into a bitmap.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace srcdsp {

// number of detected samples before sample j among det[0 .. k) (ascending)
__host__ __device__ inline int corr_all_before(const int *det, int k, long j) {
    while (k > 0 && det[k - 1] >= j) --k;
    return k;
}

// the `back`-th sample before j that is not deleted (back >= 1); kd =
// corr_all_before(det, k, j)
__host__ __device__ inline long corr_all_back(const int *det, int kd, long j, long back) {
    long p = j - back;
    for (int d = kd - 1; d >= 0 && det[d] >= p; --d) --p;
    return p;
}

// corrValue[0] and energyValue[0] after processing sample j
// (correlators.h:233-250 at S == 1, int32 wrap-around sums): tap N - 1 on j
// itself, the taps below on the samples before it with the deleted ones
// skipped.  fetch(p) is effective stream sample p of the call (p >= -(N - 1):
// input, then history).
template <class Fetch>
__host__ __device__ inline void corr_all_value(Fetch fetch, const int32_t *coef, int N, unsigned cs, const int *det,
                                               int kd, long j, uint32_t &c, uint32_t &e) {
    uint32_t tr = 0, ti = 0, en = 0;
    long p = j;
    int d = kd;
    long nd = d > 0 ? (long)det[d - 1] : -1 - (long)N;  // the next deleted sample below p (none: below the history)
    for (int m = N - 1; m >= 0; --m) {
        const uint32_t w = fetch(p);
        const int32_t hr = (int32_t)(int16_t)(w & 0xffffu), hi = (int32_t)w >> 16;
        const int32_t cr = coef[2 * m], ci = coef[2 * m + 1];
        tr += (uint32_t)hr * (uint32_t)cr - (uint32_t)hi * (uint32_t)ci;
        ti += (uint32_t)hr * (uint32_t)ci + (uint32_t)hi * (uint32_t)cr;
        en += (uint32_t)hr * (uint32_t)hr + (uint32_t)hi * (uint32_t)hi;
        --p;
        while (p == nd) {
            --p;
            --d;
            nd = d > 0 ? (long)det[d - 1] : -1 - (long)N;
        }
    }
    const int32_t sr = (int32_t)tr >> (cs & 31u), si = (int32_t)ti >> (cs & 31u);  // scale32 :244
    const int32_t ar = sr >> 2, ai = si >> 2;                                       // :250
    c = (uint32_t)ar * (uint32_t)ar + (uint32_t)ai * (uint32_t)ai;
    e = en >> ((unsigned)((int)cs / 2) & 31u);  // :245
}

// the registers tested at value t of a batch c[], e[] that follows c2, c1 (and e1)
__host__ __device__ inline void corr_all_triple(const uint32_t *c, const uint32_t *e, int t, uint32_t c2, uint32_t c1,
                                                uint32_t e1, uint32_t &a2, uint32_t &a1, uint32_t &ae) {
    a2 = t >= 2 ? c[t - 2] : (t == 1 ? c1 : c2);
    a1 = t >= 1 ? c[t - 1] : c1;
    ae = t >= 1 ? e[t - 1] : e1;
}

// first_hit of the walk, in order (the host's form; the device tests one value per lane)
template <class Hit>
__host__ __device__ inline int corr_all_first_hit(Hit hit, const uint32_t *c, const uint32_t *e, int cnt, uint32_t c2,
                                                  uint32_t c1, uint32_t e1) {
    for (int t = 0; t < cnt; ++t) {
        uint32_t a2, a1, ae;
        corr_all_triple(c, e, t, c2, c1, e1, a2, a1, ae);
        if (hit(a2, a1, c[t], ae)) return t;
    }
    return -1;
}

struct CorrAllResult {
    int hits;                     // detections made
    long consumed;                // samples the loop processed
    uint32_t corr[3], energy[3];  // the registers after sample consumed - 1
};

// The walk.  X supplies
//   long     next(long pos)         first sample >= pos where the undisturbed test fires, -1: none
//   void     eval(long j, int cnt, int k)
//                                   the registers after samples j .. j + cnt - 1 (cnt <= batch()),
//                                   each with the deletions det[0 .. k) before it, into c(t), e(t)
//   uint32_t c(int t), e(int t)
//   int      batch()
//   int      first_hit(int cnt, c2, c1, e1)
//                                   the first t < cnt at which the test of correlators.h:262-268
//                                   fires on (c(t - 2), c(t - 1), c(t), e(t - 1)), the values before
//                                   c(0) being c2, c1 and e1; -1: none
//   void     record(int k, long q)  det[k] = q, seen by the next eval
//   uint32_t pc[3], pe[3]           the registers carried into the call
// On the device every lane of the workgroup runs the walk on block-uniform
// values; eval and next are the cooperative parts.
template <class X>
__host__ __device__ inline void corr_all_walk(X &x, long n, int N, int max_hits, CorrAllResult &r) {
    int k = 0;
    long pos = 0, consumed = n;
    bool full = false;
    while (!full) {
        const long i = x.next(pos);  // the stream is undisturbed from pos on
        if (i < 0) break;
        x.record(k++, i);
        if (k == max_hits) {
            consumed = i + 1;
            break;
        }
        // the first triple of the patch: c(i - 1), c(i), then the recomputed values
        uint32_t c2, c1, e1;
        if (i >= 1) {
            x.eval(i - 1, 2, k);
            c2 = x.c(0), c1 = x.c(1), e1 = x.e(1);
        } else {
            x.eval(0, 1, k);
            c2 = x.pc[0], c1 = x.c(0), e1 = x.e(0);
        }
        long end = i + N + 1;  // the last sample whose test the deletion disturbs
        long j = i + 1;
        while (j <= end && j < n) {
            long left = (end < n - 1 ? end : n - 1) - j + 1;
            const int cnt = (int)(left < x.batch() ? left : x.batch());
            x.eval(j, cnt, k);
            const int t = x.first_hit(cnt, c2, c1, e1);
            const int used = t < 0 ? cnt : t + 1;  // values tested; the ones after a detection are stale
            c2 = used >= 2 ? x.c(used - 2) : c1;
            c1 = x.c(used - 1);
            e1 = x.e(used - 1);
            j += used;
            if (t >= 0) {  // a detection inside the patch extends it
                const long q = j - 1;
                x.record(k++, q);
                if (k == max_hits) {
                    consumed = q + 1;
                    full = true;
                    break;
                }
                end = q + N + 1;
            }
        }
        pos = end + 1;
    }
    r.hits = k;
    r.consumed = consumed;
    // the registers after the last processed sample, reaching back into the carried ones
    const long lo = consumed >= 3 ? consumed - 3 : 0;
    const int cnt = (int)(consumed - lo);
    if (cnt > 0) x.eval(lo, cnt, k);
    for (int t = 0; t < 3; ++t) {
        const long idx = consumed - 1 - t;
        r.corr[t] = idx >= 0 ? x.c((int)(idx - lo)) : x.pc[-idx - 1];
        r.energy[t] = idx >= 0 ? x.e((int)(idx - lo)) : x.pe[-idx - 1];
    }
}

}  // namespace srcdsp
