// corr_all_host.cpp -- the walk of srcdsp_corr_step_all (csrc/corr_all_walk.h)
// compiled for the host, with the candidate bitmap built by a plain loop and
// the reference's literal sqrt test (correlators.h:262-268; host sqrt is
// correctly rounded).  Stand-alone, so the sanitisers see every index the walk
// forms.
//
//   corr_all_host N cs max_hits batch pattern.bin in.bin n1 n2 ...
//
// pattern.bin: N complex<int32_t>; in.bin: complex<int16_t> samples, taken in
// calls of n1, n2, ... (a call that stops at max_hits is followed by calls on
// its remainder).  Per call it prints
//   H hits consumed corr[0..2] energy[0..2]
//   I corrIndex ...
//   B re im ...            one line per detection (bitSamples)
// and at the end  T re im ...  (the history).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "corr_all_walk.h"

using namespace srcdsp;

static std::vector<char> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<char> b;
    char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}

static bool ref_hit(uint32_t c2, uint32_t c1, uint32_t c0, uint32_t e1) {
    if (c1 > c2 && c1 > c0) {
        double corr = sqrt((double)c1);
        double energy = sqrt((double)e1);
        if (corr > energy * 2.7 && energy > 300) return true;
    }
    return false;
}

struct Fetch {
    const uint32_t *in, *hist;
    long n, NSm1;
    uint32_t operator()(long p) const {
        if (p >= n || p < -NSm1) abort();  // the walk never reads outside the stream
        return p >= 0 ? in[p] : hist[p + NSm1];
    }
};

struct HostX {
    Fetch fetch;
    const int32_t *coef;
    int N, B;
    unsigned cs;
    long n;
    std::vector<uint64_t> map;
    std::vector<int> det;
    std::vector<uint32_t> cb, eb;
    uint32_t pc[3], pe[3];

    long next(long pos) const {
        for (long i = pos; i < n; ++i)
            if (map[(size_t)(i >> 6)] >> (i & 63) & 1) return i;
        return -1;
    }
    void eval(long j, int cnt, int k) {
        if (cnt > B) abort();
        for (int t = 0; t < cnt; ++t)
            corr_all_value(fetch, coef, N, cs, det.data(), corr_all_before(det.data(), k, j + t), j + t, cb[(size_t)t],
                           eb[(size_t)t]);
        for (int t = cnt; t < B; ++t) cb[(size_t)t] = eb[(size_t)t] = 0xdeadbeefu;
    }
    uint32_t c(int t) const { return cb.at((size_t)t); }
    uint32_t e(int t) const { return eb.at((size_t)t); }
    int batch() const { return B; }
    int first_hit(int cnt, uint32_t c2, uint32_t c1, uint32_t e1) const {
        return corr_all_first_hit(ref_hit, cb.data(), eb.data(), cnt, c2, c1, e1);
    }
    void record(int k, long q) { det.at((size_t)k) = (int)q; }
};

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    const int N = atoi(argv[1]);
    const unsigned cs = (unsigned)atoi(argv[2]);
    const int max_hits = atoi(argv[3]), B = atoi(argv[4]);
    std::vector<char> pb = slurp(argv[5]), xb = slurp(argv[6]);
    if (pb.size() != 8 * (size_t)N || B < 3 || max_hits < 1) return 2;
    const int32_t *p = (const int32_t *)pb.data();
    std::vector<int32_t> coef(2 * (size_t)N);
    for (int m = 0; m < N; ++m) {  // conjugate (correlators.h:173-176)
        coef[2 * (size_t)m] = p[2 * m];
        coef[2 * (size_t)m + 1] = -p[2 * m + 1];
    }
    const uint32_t *x = (const uint32_t *)xb.data();
    const long total = (long)(xb.size() / 4);
    const long NSm1 = N - 1;
    std::vector<uint32_t> hist((size_t)(NSm1 > 0 ? NSm1 : 1), 0u);
    uint32_t corr[3] = {0, 0, 0}, energy[3] = {0, 0, 0};
    long pos = 0;
    for (int a = 7; a < argc; ++a) {
        long left = atol(argv[a]);
        if (pos + left > total) return 2;
        while (left > 0) {
            const long n = left;
            // an exact-size copy of the call's input: a read past it is a heap overflow
            std::vector<uint32_t> in(x + pos, x + pos + n);
            HostX X;
            X.fetch = Fetch{in.data(), hist.data(), n, NSm1};
            X.coef = coef.data();
            X.N = N;
            X.B = B;
            X.cs = cs;
            X.n = n;
            X.det.assign((size_t)max_hits, -1);
            X.cb.assign((size_t)B, 0);
            X.eb.assign((size_t)B, 0);
            for (int k = 0; k < 3; ++k) {
                X.pc[k] = corr[k];
                X.pe[k] = energy[k];
            }
            // candidates: the test on the stream with nothing deleted
            X.map.assign((size_t)((n + 63) / 64), 0);
            {
                uint32_t c2 = corr[1], c1 = corr[0], e1 = energy[0];
                for (long i = 0; i < n; ++i) {
                    uint32_t c0, e0;
                    corr_all_value(X.fetch, coef.data(), N, cs, X.det.data(), 0, i, c0, e0);
                    if (ref_hit(c2, c1, c0, e1)) X.map[(size_t)(i >> 6)] |= 1ull << (i & 63);
                    c2 = c1, c1 = c0, e1 = e0;
                }
            }
            CorrAllResult r;
            corr_all_walk(X, n, N, max_hits, r);
            printf("H %d %ld %u %u %u %u %u %u\nI", r.hits, r.consumed, r.corr[0], r.corr[1], r.corr[2], r.energy[0],
                   r.energy[1], r.energy[2]);
            for (int h = 0; h < r.hits; ++h) printf(" %d", X.det[(size_t)h] - 1);
            printf("\n");
            for (int h = 0; h < r.hits; ++h) {
                printf("B");
                const long q = X.det[(size_t)h];
                for (int m = 0; m < N; ++m) {
                    const uint32_t w = X.fetch(m == 0 ? q : corr_all_back(X.det.data(), h, q, N - m));
                    printf(" %d %d", (int)(int16_t)(w & 0xffffu), (int)(int16_t)(w >> 16));
                }
                printf("\n");
            }
            std::vector<uint32_t> nh(hist.size(), 0u);
            for (long k = 0; k < NSm1; ++k)
                nh[(size_t)k] = X.fetch(corr_all_back(X.det.data(), r.hits, r.consumed, NSm1 - k));
            hist = nh;
            for (int k = 0; k < 3; ++k) {
                corr[k] = r.corr[k];
                energy[k] = r.energy[k];
            }
            if (r.consumed < 1 || r.consumed > n) return 3;
            pos += r.consumed;
            left -= r.consumed;
        }
    }
    printf("T");
    for (long k = 0; k < NSm1; ++k)
        printf(" %d %d", (int)(int16_t)(hist[(size_t)k] & 0xffffu), (int)(int16_t)(hist[(size_t)k] >> 16));
    printf("\n");
    return 0;
}
