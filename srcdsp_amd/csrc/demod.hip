// demod.hip -- dsptl::DemodulatorOqpsk<int16_t> (demodulators.h:53-130,
// demodulators.cpp:34-308) on gfx950: srcdsp_demod_step and the bank
// srcdsp_demod_step_batched, one kernel for both (the single step is the bank
// at one channel).
//
// The PLL makes a burst a loop-carried recurrence; C bursts are C independent
// ones.  demod_bank gives every burst a lane (demod_kernels.h): all integer,
// so every channel is bit for bit the reference's step().
//
// A handle is a host object: the configuration (pattern, reference vector,
// frequency word, shift) and StateVar, 7 words.  A call packs, per channel,
// the configuration, the state and the reference samples its preamble reads
// into one table, uploads it in one copy, launches once, and takes one packed
// row per channel back (new state, error, accumulatedFrequency) after its one
// synchronisation.  The call returns with its stream synchronised (the error
// is needed on the host), so the steps of a handle are ordered on any streams
// without an event.  The table and the rows live on hs[0] and grow on demand.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "ops.h"
#include "corr_state.h"
#include "demod_kernels.h"
#include "freqest_pair.h"

namespace srcdsp {

constexpr double kDemodPi = 3.141592653589793238462643383279502884197169399375105820974944592307816406286;
static_assert(kDemodLdsBytes == 71424, "DESIGN 5.5 and tests/test_demod_capi.py quote the workgroup's LDS");
static_assert(sizeof(DemodChan) % 8 == 0, "the reference samples follow the table, 4-byte aligned");

__global__ __launch_bounds__(kDemodLanes) void demod_bank(const DemodChan *__restrict__ chan, int channels,
                                                          const uint32_t *__restrict__ refs,
                                                          const uint32_t *__restrict__ in, long n,
                                                          int8_t *__restrict__ soft,
                                                          const uint32_t *__restrict__ tables,
                                                          int32_t *__restrict__ res) {
    constexpr int T = kDemodTile, L = kDemodLanes;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kDemodLdsBytes / 4];
    const int16_t *sine = (const int16_t *)lds, *phase_lut = sine + kDemodSine;
    uint32_t *tile = lds + kDemodTableWords;                // [L][T + 1]
    int8_t *stile = (int8_t *)(tile + L * (T + 1));         // [L][kDemodSoftStride]
    long *row_in = (long *)(stile + L * kDemodSoftStride);  // first input sample of row r
    long *row_soft = row_in + L;                            // next soft bit of row r
    uint32_t *row_cnt = (uint32_t *)(row_soft + L);         // soft bits of row r in this tile
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * L;
    const int rows = min(L, channels - c0);
    const bool active = lane < rows;

    for (int i = lane; i < kDemodTableWords / 4; i += L) ((uint4 *)lds)[i] = ((const uint4 *)tables)[i];
    DemodChan ch{};
    if (active) ch = chan[c0 + lane];
    row_in[lane] = ch.in_off;
    DemodLane s{(uint32_t)ch.st[DS_BITCNT], ch.st[DS_MOD2], ch.st[DS_PHASE], ch.st[DS_BIT1], ch.st[DS_BIT2],
                ch.st[DS_IPREV], ch.st[DS_QPREV], 0u, 0};
    long sc = 0;  // soft bits this row has produced
    const uint32_t *ref = refs + ch.ref_off;
    const long acc_from = n >= 32 ? n - 32 : n;  // freqComputationStart (:181, :264)
    __syncthreads();

    // tile t + 1 is in flight (registers) while tile t is computed
    uint32_t pre[L];
    auto load = [&](long k0) {
        const long k = k0 + lane;
#pragma unroll
        for (int r = 0; r < L; ++r) pre[r] = (r < rows && k < n) ? in[row_in[r] + k] : 0u;
    };
    load(0);
    for (long k0 = 0; k0 < n; k0 += T) {
#pragma unroll
        for (int r = 0; r < L; ++r) tile[r * (T + 1) + lane] = pre[r];
        __syncthreads();
        if (k0 + T < n) load(k0 + T);
        const int kmax = (int)min((long)T, n - k0);
        int tc = 0;
        if (active) {
            for (int k = 0; k < kmax; ++k) {
                const long kk = k0 + k;
                uint32_t rw = 0;
                if (ch.P != 0 && s.bit_cnt + 1 < (uint32_t)ch.P && kk < ch.ref_len) rw = ref[kk];
                int sv = 0;
                if (demod_sample(s, tile[lane * (T + 1) + k], rw, (unsigned)ch.P, ch.shift, ch.freq, kk >= acc_from,
                                 sine, phase_lut, &sv))
                    stile[lane * kDemodSoftStride + tc++] = (int8_t)sv;
            }
        }
        row_soft[lane] = ch.soft_off + sc;
        row_cnt[lane] = (uint32_t)tc;
        sc += tc;
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            if (lane < (int)row_cnt[r]) soft[row_soft[r] + lane] = stile[r * kDemodSoftStride + lane];
        __syncthreads();
    }
    if (!active) return;
    // a vector sized n of which fewer were written (a call inside the
    // preamble that is not the first): the rest as the reference's assign({})
    for (long j = sc; j < ch.soft_len; ++j) soft[ch.soft_off + j] = 0;
    int32_t *row = res + (long)DS_WORDS * (c0 + lane);
    row[DS_BITCNT] = (int32_t)s.bit_cnt;
    row[DS_MOD2] = s.mod2;
    row[DS_PHASE] = s.phase;
    row[DS_BIT1] = s.bit1;
    row[DS_BIT2] = s.bit2;
    row[DS_IPREV] = s.i_prev;
    row[DS_QPREV] = s.q_prev;
    row[DS_ERROR] = (int32_t)s.err_acc;
    row[DS_ACCFREQ] = s.acc_freq;
}

struct DemodState {
    std::vector<int8_t> pattern;   // bitSyncPattern, 0 / 1
    std::vector<uint32_t> ref;     // packed (Iref, Qref)
    int freq = 0, init_phase = 0;  // intialFreqEst, initialPhase (stored only)
    int shift = 0;                 // rightShift
    int acc_freq = 0;              // accumulatedFrequency
    int32_t st[7] = {0, 0, 0, 0, 0, 0, 0};  // StateVar, DS_BITCNT .. DS_QPREV
    // scratch of the calls this handle led: the table on the device and its
    // pinned host image, the result rows likewise
    GrowBuf tab, res;
    HostStage stage;     // srcdsp_demod_step_host

    void reset() {  // demodulators.cpp:293-308
        for (int &v : st) v = 0;
        shift = 0;
        if (!pattern.empty()) {
            st[DS_BIT1] = 2 * pattern[pattern.size() - 1] - 1;
            st[DS_BIT2] = 2 * pattern[pattern.size() - 2] - 1;
        }
    }
};

namespace {

// the constructor's tables (demodulators.cpp:39-55), the reference's own
// expressions in double: sine 8192 | phase 128 x 128
const int16_t *demod_host_tables() {
    static const std::vector<int16_t> t = [] {
        std::vector<int16_t> v(kDemodSine + kDemodPhase);
        for (int index = 0; index < kDemodSine; ++index) {
            const double phase = index * (kDemodPi / static_cast<double>(4096));
            v[index] = static_cast<int16_t>(std::sin(phase) * INT16_MAX);
        }
        for (int im = 0; im < kDemodAmp; ++im)
            for (int re = 0; re < kDemodAmp; ++re)
                v[kDemodSine + im * kDemodAmp + re] =
                    static_cast<int16_t>(std::round(std::atan2((double)im, (double)re) * 4096 / kDemodPi));
        return v;
    }();
    return t.data();
}

// one device copy per device, process-wide, made at the first step
int demod_device_tables(const uint32_t **out) {
    static std::mutex mu;
    static std::map<int, uint32_t *> copies;
    int dev = 0;
    SRCDSP_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = copies.find(dev);
    if (it == copies.end()) {
        uint32_t *d = nullptr;
        SRCDSP_HIP_TRY(hipMalloc(&d, 4 * (size_t)kDemodTableWords));
        hipError_t e = hipMemcpy(d, demod_host_tables(), 4 * (size_t)kDemodTableWords, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            set_error(std::string("demod tables: ") + hipGetErrorString(e));
            return SRCDSP_ERR_HIP;
        }
        it = copies.emplace(dev, d).first;
    }
    *out = it->second;
    return SRCDSP_OK;
}

// float rad/sample -> the table's frequency word (setInitialFrequency,
// demodulators.h:64): the product in float, the division and round() in
// double.  False for a word outside +-4096, which lets the reference's phase go
// negative (phaseShift asserts, :109).
bool demod_freq_word(float f, int *word) {
    const double w = std::round((double)(f * (float)4096) / kDemodPi);
    if (!(w >= -4096.0 && w <= 4096.0)) return false;
    *word = (int)w;
    return true;
}

// soft bits of a call of n samples (:167-175), and the reference samples its
// preamble reads (Iref[k], k the index within the call, while bitCnt < P)
size_t demod_n_soft(const DemodState &d, size_t n) {
    return d.st[DS_BITCNT] == 0 && !d.pattern.empty() ? n - d.pattern.size() : n;
}
size_t demod_ref_reads(const DemodState &d, size_t n) {
    const size_t P = d.pattern.size(), b0 = (uint32_t)d.st[DS_BITCNT];
    return P > b0 + 1 ? std::min(n, P - 1 - b0) : 0;
}

}  // namespace
}  // namespace srcdsp

struct srcdsp_demod { srcdsp::DemodState d; };

using namespace srcdsp;

namespace {

// every check of a call, before anything changes: SRCDSP_OK or the refusal
int demod_check(const srcdsp_demod_t *hs, int channels, size_t n, const char *who) {
    for (int c = 0; c < channels; ++c) {
        const DemodState &d = hs[c]->d;
        if (d.st[DS_BITCNT] == 0 && !d.pattern.empty() && n <= d.pattern.size()) {
            set_error(std::string(who) + ": the first call needs more samples than the sync pattern has bits "
                                         "(demodulators.cpp:171 asserts)");
            return SRCDSP_ERR_SIZE;
        }
        if (demod_ref_reads(d, n) > d.ref.size()) {
            set_error(std::string(who) + ": the reference vector is shorter than the preamble "
                                         "(demodulators.cpp:196 reads past Iref)");
            return SRCDSP_ERR_SIZE;
        }
    }
    return SRCDSP_OK;
}

// the checked call: table up, one launch, rows back, handles updated
int demod_run(const srcdsp_demod_t *hs, int channels, const uint32_t *d_in, size_t in_stride,
              const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride, int32_t *error,
              hipStream_t s) {
    DemodState &lead = hs[0]->d;
    const size_t C = (size_t)channels;
    size_t ref_words = 0;
    for (size_t c = 0; c < C; ++c) ref_words += demod_ref_reads(hs[c]->d, n);
    const size_t tab_bytes = C * sizeof(DemodChan) + 4 * ref_words;
    int rc = lead.tab.reserve(tab_bytes);
    if (!rc) rc = lead.res.reserve(4 * DS_WORDS * C);
    if (rc) return rc;
    const DemodChan *d_tab = lead.tab.dev<DemodChan>();
    int32_t *d_res = lead.res.dev<int32_t>(), *h_res = lead.res.host<int32_t>();
    const uint32_t *d_tables = nullptr;
    rc = demod_device_tables(&d_tables);
    if (rc) return rc;
    DemodChan *tab = lead.tab.host<DemodChan>();
    uint32_t *refs = (uint32_t *)(tab + C);
    size_t ref_at = 0;
    for (size_t c = 0; c < C; ++c) {
        const DemodState &d = hs[c]->d;
        DemodChan &t = tab[c];
        t.in_off = (long)(c * in_stride + (in_offset ? in_offset[c] : 0));
        t.soft_off = (long)(c * soft_stride);
        t.soft_len = (long)demod_n_soft(d, n);
        t.ref_off = (int)ref_at;
        t.ref_len = (int)demod_ref_reads(d, n);
        t.P = (int)d.pattern.size();
        t.shift = d.shift;
        t.freq = d.freq;
        for (int k = 0; k < 7; ++k) t.st[k] = d.st[k];
        if (t.ref_len) memcpy(refs + ref_at, d.ref.data(), 4 * (size_t)t.ref_len);
        ref_at += (size_t)t.ref_len;
    }
    SRCDSP_HIP_TRY(hipMemcpyAsync(lead.tab.d, tab, tab_bytes, hipMemcpyHostToDevice, s));
    const unsigned blocks = (unsigned)((C + kDemodLanes - 1) / kDemodLanes);
    hipLaunchKernelGGL(demod_bank, dim3(blocks), dim3(kDemodLanes), 0, s, d_tab, channels,
                       (const uint32_t *)(d_tab + C), d_in, (long)n, d_soft, d_tables, d_res);
    SRCDSP_HIP_TRY(hipGetLastError());
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_res, d_res, 4 * DS_WORDS * C, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    for (size_t c = 0; c < C; ++c) {
        DemodState &d = hs[c]->d;
        const int32_t *row = h_res + DS_WORDS * c;
        for (int k = 0; k < 7; ++k) d.st[k] = row[k];
        d.acc_freq = row[DS_ACCFREQ];
        error[c] = row[DS_ERROR];
    }
    return SRCDSP_OK;
}

}  // namespace

extern "C" {

// ctor (demodulators.cpp:34-58): the tables are process-wide here
SRCDSP_API int srcdsp_demod_create(srcdsp_demod_t *out) {
    SRCDSP_ARG_CHECK(out != nullptr, "demod_create: null out");
    *out = new srcdsp_demod();
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_destroy(srcdsp_demod_t h) {
    if (!h) return SRCDSP_OK;
    DemodState &d = h->d;
    d.tab.destroy();
    d.res.destroy();
    if (d.stage.stream) d.stage.destroy();
    delete h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_clone(srcdsp_demod_t h, srcdsp_demod_t *out) {
    SRCDSP_ARG_CHECK(h != nullptr && out != nullptr, "demod_clone: null argument");
    auto *n = new srcdsp_demod();
    const DemodState &s = h->d;
    DemodState &d = n->d;
    d.pattern = s.pattern;
    d.ref = s.ref;
    d.freq = s.freq;
    d.init_phase = s.init_phase;
    d.shift = s.shift;
    d.acc_freq = s.acc_freq;
    for (int k = 0; k < 7; ++k) d.st[k] = s.st[k];
    *out = n;
    return SRCDSP_OK;
}

// setSyncPattern (demodulators.h:60)
SRCDSP_API int srcdsp_demod_set_sync_pattern(srcdsp_demod_t h, const int8_t *bits, int nbits) {
    SRCDSP_ARG_CHECK(h != nullptr && nbits >= 0 && (bits != nullptr || nbits == 0), "demod_set_sync_pattern: null argument");
    SRCDSP_ARG_CHECK(nbits != 1, "demod_set_sync_pattern: a pattern has at least 2 bits (demodulators.cpp:302 asserts)");
    for (int k = 0; k < nbits; ++k)
        SRCDSP_ARG_CHECK(bits[k] == 0 || bits[k] == 1, "demod_set_sync_pattern: bits are 0 or 1 (demodulators.h:94)");
    h->d.pattern.assign(bits, bits + nbits);
    return SRCDSP_OK;
}

// setReference (demodulators.cpp:126-139)
SRCDSP_API int srcdsp_demod_set_reference(srcdsp_demod_t h, const int16_t *ref_host, int n) {
    SRCDSP_ARG_CHECK(h != nullptr && n >= 0 && (ref_host != nullptr || n == 0), "demod_set_reference: null argument");
    h->d.ref.resize((size_t)n);
    if (n) memcpy(h->d.ref.data(), ref_host, 4 * (size_t)n);
    return SRCDSP_OK;
}

// setReference(corr.getRefBitSamples()) (correlators.h:311-316) without the
// caller's vector: the correlator's step is synchronous and leaves bitSamples
// in its handle, from where they are taken
SRCDSP_API int srcdsp_demod_set_reference_corr(srcdsp_demod_t h, srcdsp_corr_t corr, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && corr != nullptr, "demod_set_reference_corr: null argument");
    (void)stream;
    int rc = corr->c.order.sync();
    if (rc) return rc;
    h->d.ref.resize(corr->c.N);
    memcpy(h->d.ref.data(), corr->c.bits.data(), 4 * (size_t)corr->c.N);
    return SRCDSP_OK;
}

// setInitialFrequency (demodulators.h:64)
SRCDSP_API int srcdsp_demod_set_initial_frequency(srcdsp_demod_t h, float f) {
    int word = 0;
    SRCDSP_ARG_CHECK(demod_freq_word(f, &word), "demod_set_initial_frequency: frequency word outside +-4096");
    SRCDSP_ARG_CHECK(h != nullptr, "demod_set_initial_frequency: null handle");
    h->d.freq = word;
    return SRCDSP_OK;
}

// setInitialPhase (demodulators.h:66): stored, never used by step()
SRCDSP_API int srcdsp_demod_set_initial_phase(srcdsp_demod_t h, float p) {
    const double w = std::round((double)(p * (float)4096) / kDemodPi);
    SRCDSP_ARG_CHECK(w >= -32768.0 && w <= 32767.0, "demod_set_initial_phase: phase word outside int16");
    SRCDSP_ARG_CHECK(h != nullptr, "demod_set_initial_phase: null handle");
    h->d.init_phase = (int)w;
    return SRCDSP_OK;
}

// setInputShift (demodulators.h:70)
SRCDSP_API int srcdsp_demod_set_input_shift(srcdsp_demod_t h, int shift) {
    SRCDSP_ARG_CHECK(h != nullptr, "demod_set_input_shift: null handle");
    SRCDSP_ARG_CHECK(shift >= 0 && shift <= 15, "demod_set_input_shift: shift outside 0..15");
    h->d.shift = shift;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_reset(srcdsp_demod_t h) {
    SRCDSP_ARG_CHECK(h != nullptr, "demod_reset: null handle");
    h->d.reset();
    return SRCDSP_OK;
}

// getMeasuredFrequency (demodulators.h:72)
SRCDSP_API int srcdsp_demod_get_measured_frequency(srcdsp_demod_t h, float *f) {
    SRCDSP_ARG_CHECK(h != nullptr && f != nullptr, "demod_get_measured_frequency: null argument");
    *f = static_cast<float>((h->d.acc_freq >> 5) * kDemodPi / 4096);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_get_state(srcdsp_demod_t h, unsigned *bit_cnt, int *mod2_cnt, int *phase, int *bit1,
                                      int *bit2, int *i_prev, int *q_prev, int *freq_word, int *acc_freq, int *shift) {
    SRCDSP_ARG_CHECK(h != nullptr, "demod_get_state: null handle");
    const DemodState &d = h->d;
    if (bit_cnt) *bit_cnt = (unsigned)d.st[DS_BITCNT];
    if (mod2_cnt) *mod2_cnt = d.st[DS_MOD2];
    if (phase) *phase = d.st[DS_PHASE];
    if (bit1) *bit1 = d.st[DS_BIT1];
    if (bit2) *bit2 = d.st[DS_BIT2];
    if (i_prev) *i_prev = d.st[DS_IPREV];
    if (q_prev) *q_prev = d.st[DS_QPREV];
    if (freq_word) *freq_word = d.freq;
    if (acc_freq) *acc_freq = d.acc_freq;
    if (shift) *shift = d.shift;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_get_tables(int16_t *sine8192_host, int16_t *phase16384_host) {
    const int16_t *t = demod_host_tables();
    if (sine8192_host) memcpy(sine8192_host, t, 2 * (size_t)kDemodSine);
    if (phase16384_host) memcpy(phase16384_host, t + kDemodSine, 2 * (size_t)kDemodPhase);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_demod_step_batched(const srcdsp_demod_t *hs, int channels, const void *d_in, size_t in_stride,
                                         const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride,
                                         size_t *n_soft, int32_t *error, void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && n_soft != nullptr && error != nullptr && channels >= 1,
                     "demod_step_batched: no handles or result arrays");
    int rc = check_handles(hs, channels, "demod_step_batched");
    if (rc) return rc;
    if (n > 0x7fffffffUL) {
        set_error("demod_step_batched: input longer than INT_MAX samples (demodulators.cpp:181 uses int)");
        return SRCDSP_ERR_SIZE;
    }
    if (n == 0) {
        for (int c = 0; c < channels; ++c) {
            n_soft[c] = 0;
            error[c] = 0;
        }
        return SRCDSP_OK;
    }
    SRCDSP_ARG_CHECK(d_in != nullptr && d_soft != nullptr, "demod_step_batched: null buffer");
    rc = demod_check(hs, channels, n, "demod_step_batched");
    if (rc) return rc;
    for (int c = 0; c < channels; ++c)
        if (demod_n_soft(hs[c]->d, n) > soft_stride) {
            set_error("demod_step_batched: soft_stride smaller than a channel's soft bits");
            return SRCDSP_ERR_SIZE;
        }
    for (int c = 0; c < channels; ++c) n_soft[c] = demod_n_soft(hs[c]->d, n);
    return demod_run(hs, channels, (const uint32_t *)d_in, in_stride, in_offset, n, d_soft, soft_stride, error,
                     (hipStream_t)stream);
}

SRCDSP_API int srcdsp_demod_step(srcdsp_demod_t h, const void *d_in, size_t n, int8_t *d_soft, size_t cap,
                                 size_t *n_soft, int32_t *error, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && n_soft != nullptr && error != nullptr, "demod_step: null argument");
    return srcdsp_demod_step_batched(&h, 1, d_in, 0, nullptr, n, d_soft, cap, n_soft, error, stream);
}

SRCDSP_API int srcdsp_demod_step_host(srcdsp_demod_t h, const void *in, size_t n, int8_t *soft, size_t cap,
                                      size_t *n_soft, int32_t *error) {
    SRCDSP_ARG_CHECK(h != nullptr && n_soft != nullptr && error != nullptr, "demod_step_host: null argument");
    if (n > 0x7fffffffUL) {
        set_error("demod_step_host: input longer than INT_MAX samples (demodulators.cpp:181 uses int)");
        return SRCDSP_ERR_SIZE;
    }
    *n_soft = 0;
    *error = 0;
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(in != nullptr && soft != nullptr, "demod_step_host: null buffer");
    int rc = demod_check(&h, 1, n, "demod_step_host");
    if (rc) return rc;
    DemodState &d = h->d;
    const size_t ns = demod_n_soft(d, n);
    if (ns > cap) {
        set_error("demod_step_host: cap smaller than the call's soft bits");
        return SRCDSP_ERR_SIZE;
    }
    if (!d.stage.stream) {
        rc = d.stage.init();
        if (rc) return rc;
    }
    rc = d.stage.reserve(5 * n, 5 * n);  // samples, then soft bits
    if (rc) return rc;
    host_copy(d.stage.h_buf, in, 4 * n);
    SRCDSP_HIP_TRY(hipMemcpyAsync(d.stage.d_buf, d.stage.h_buf, 4 * n, hipMemcpyHostToDevice, d.stage.stream));
    int8_t *d_soft = (int8_t *)d.stage.d_buf + 4 * n, *h_soft = (int8_t *)d.stage.h_buf + 4 * n;
    rc = demod_run(&h, 1, (const uint32_t *)d.stage.d_buf, 0, nullptr, n, d_soft, ns, error, d.stage.stream);
    if (rc) return rc;
    if (ns) {
        SRCDSP_HIP_TRY(hipMemcpyAsync(h_soft, d_soft, ns, hipMemcpyDeviceToHost, d.stage.stream));
        SRCDSP_HIP_TRY(hipStreamSynchronize(d.stage.stream));
        memcpy(soft, h_soft, ns);
    }
    *n_soft = ns;
    return SRCDSP_OK;
}

// The join of the correlator bank and the demodulator bank: per taken channel
// setReference(corr.getRefBitSamples()), estimateFreq<int16_t, L>
// (dsptl_miscellaneous.h:43-58) over bit samples first .. N - 1,
// setInitialFrequency(scale * est), reset().  The bit samples are in the
// correlator's host-side handle, so nothing is launched: the estimate is
// freqest_pair, the kernel's per-pair arithmetic, on the host.  Every check
// comes before the first handle changes.
SRCDSP_API int srcdsp_demod_acquire_batched(const srcdsp_demod_t *demods, const srcdsp_corr_t *cors, int channels,
                                            const int *found, int L, int first, float scale, float *freq) {
    SRCDSP_ARG_CHECK(demods != nullptr && cors != nullptr, "demod_acquire_batched: no handles");
    SRCDSP_ARG_CHECK(channels >= 1, "demod_acquire_batched: channels is at least 1");
    SRCDSP_ARG_CHECK(L >= 1, "demod_acquire_batched: L is at least 1");
    std::vector<const void *> taken;
    for (int c = 0; c < channels; ++c) {
        if (found && !found[c]) continue;
        SRCDSP_ARG_CHECK(demods[c] != nullptr && cors[c] != nullptr, "demod_acquire_batched: null handle");
        SRCDSP_ARG_CHECK(first >= 0 && (unsigned)first < cors[c]->c.N,
                         "demod_acquire_batched: first outside 0..N-1 of a correlator");
        taken.push_back(demods[c]);
    }
    int rc = check_handle_list(taken, "demod_acquire_batched", "demodulator");
    if (rc) return rc;
    std::vector<float> est((size_t)channels, 0.0f);
    std::vector<int> word((size_t)channels, 0);
    for (int c = 0; c < channels; ++c) {
        if (found && !found[c]) continue;
        srcdsp_corr_state &k = cors[c]->c;
        rc = k.order.sync();
        if (rc) return rc;
        const FreqAcc a = freqest_row_host((const uint32_t *)k.bits.data() + first, k.N - (size_t)first, (size_t)L);
        est[c] = static_cast<float>(std::atan2((double)a.sq, (double)a.si) / L);
        SRCDSP_ARG_CHECK(demod_freq_word(scale * est[c], &word[c]),
                         "demod_acquire_batched: frequency word outside +-4096");
    }
    for (int c = 0; c < channels; ++c) {
        if (found && !found[c]) continue;
        DemodState &d = demods[c]->d;
        const srcdsp_corr_state &k = cors[c]->c;
        d.ref.resize(k.N);
        memcpy(d.ref.data(), k.bits.data(), 4 * (size_t)k.N);
        d.freq = word[c];
        d.reset();
        if (freq) freq[c] = est[c];
    }
    return SRCDSP_OK;
}

}  // extern "C"
