// bank_host.h -- the host-side frame shared by the "C channels in one call"
// entry points (srcdsp_*_batched) and the handles behind them: the handle-list
// check, grow-only scratch, path counters and the per-channel pieces of a
// chunk launch.  Host code only; the definitions that are not trivially inline
// are in runtime.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <vector>

namespace srcdsp {

// ------------------------------------------------------------ handle lists
// "Every handle non-null and listed once": SRCDSP_OK, or SRCDSP_ERR_ARG with
// "<who>: null handle" / "<who>: every <what> may be listed once".  Checks the
// list it is given (sorted in place), before anything is enqueued.
int check_handle_list(std::vector<const void *> &hv, const char *who, const char *what);

template <typename H>
int check_handles(H *const *hs, int n, const char *who, const char *what = "handle") {
    std::vector<const void *> hv(hs, hs + n);
    return check_handle_list(hv, who, what);
}

// ------------------------------------------------------- grow-only scratch
// A device buffer, a pinned host buffer, or a device buffer with a pinned
// mirror of the same size.  reserve() keeps what it has while it is large
// enough; growing frees first and drops the contents.  Pointers and capacity
// are zeroed before allocating, so a failed allocation leaves an empty buffer.
struct GrowBuf {
    enum Kind { kDevice = 1, kPinned = 2, kMirrored = kDevice | kPinned };
    explicit GrowBuf(Kind k = kMirrored) : kind(k) {}
    GrowBuf(const GrowBuf &) = delete;  // owns its buffers; freed by destroy(), as the handles free theirs
    int reserve(size_t bytes);
    void destroy();
    template <typename T> T *dev() const { return (T *)d; }
    template <typename T> T *host() const { return (T *)h; }

    Kind kind;
    void *d = nullptr, *h = nullptr;
    size_t cap = 0;  // bytes
};

// ----------------------------------------------------------- path counters
// calls served by one dispatch path since the process started (*_stats)
struct PathCounter {
    std::atomic<unsigned long> n{0};
    void hit() { n.fetch_add(1, std::memory_order_relaxed); }
    void read(unsigned long *out) const {
        if (out) *out = n.load(std::memory_order_relaxed);
    }
};

// ------------------------------------------------------------- chunk frame
// One channel's part of a launch, for a handle state S with an Ordering
// `order` and ping-pong history buffers `d_hist[2]` / `cur`: chan_begin makes
// the stream wait for the handle's previous step and names the history the
// step reads and the one it writes; chan_commit, once the launch is enqueued,
// makes the written one current and records the step.
template <typename S, typename In, typename Out>
void hist_pair(const S &st, In &in, Out &out) {
    in = (In)st.d_hist[st.cur];
    out = (Out)st.d_hist[st.cur ^ 1];
}
template <typename S, typename In, typename Out>
int chan_begin(S &st, hipStream_t s, In &in, Out &out) {
    hist_pair(st, in, out);
    return st.order.before(s);
}
template <typename S>
int chan_commit(S &st, hipStream_t s) {
    st.cur ^= 1;
    return st.order.after(s);
}

// row c of a [channels][stride] array of `es`-byte samples (stride 0: one row
// shared by every channel)
inline const void *chan_row(const void *p, size_t c, size_t stride, size_t es = 4) {
    return (const char *)p + c * stride * es;
}
inline void *chan_row(void *p, size_t c, size_t stride, size_t es = 4) { return (char *)p + c * stride * es; }

}  // namespace srcdsp
