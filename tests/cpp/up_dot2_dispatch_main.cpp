// up_dot2_dispatch_main.cpp -- the shape dispatcher of the v_dot2 transmit
// tiles (srcdsp_amd/csrc/up_dot2_dispatch.h) checked on the host, built with
// -fsanitize=address,undefined by tests/test_upmix_capi.py.
//
// For each of the three families' shape tables, every L = 1..9 and every
// PP = 1..2048: the callback runs exactly once where the family has a kernel of
// ratio L and not at all otherwise, and the <LR, PPC> it is given is the one
// the tables below say, which are written out here a second time on purpose.
#include <cstdio>

#include "../../srcdsp_amd/csrc/up_dot2_dispatch.h"

using namespace srcdsp;

static long fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (fails++ < 20) {                            \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

struct Want {
    const char *name;
    unsigned ratios;        // bit L: the family has kernels of ratio L
    int compiled[8][2];     // (L, PP) with PP compiled in, ended by (0, 0)
    int kernels;            // instantiations in all
};

static const Want kStandard = {"standard", 0x1fc, {{2, 8}, {2, 16}, {2, 32}, {4, 8}, {4, 16}, {4, 32}, {8, 8}, {8, 16}}, 15};
static const Want kResampler = {"resampler", 0x1fc, {{2, 16}, {4, 16}, {8, 8}, {0, 0}}, 10};
static const Want kSumming = {"summing tile", 0x114, {{2, 8}, {2, 16}, {2, 32}, {4, 8}, {4, 16}, {4, 32}, {8, 8}, {0, 0}}, 10};

static int want_ppc(const Want &w, unsigned L, int PP) {
    for (int i = 0; i < 8 && w.compiled[i][0]; ++i)
        if ((unsigned)w.compiled[i][0] == L && w.compiled[i][1] == PP) return PP;
    return 0;
}

template <class SHAPES>
static long sweep(const Want &w) {
    long cases = 0;
    bool seen[10][33] = {};
    for (unsigned L = 1; L <= 9; ++L)
        for (int PP = 1; PP <= 2048; ++PP, ++cases) {
            int calls = 0, lr = -1, ppc = -1;
            const bool served = up_dot2_dispatch<SHAPES>(L, PP, [&](auto l, auto p) {
                static_assert(SHAPES::has(decltype(l)::value, decltype(p)::value), "only shapes the family has");
                ++calls;
                lr = decltype(l)::value;
                ppc = decltype(p)::value;
            });
            const bool has_ratio = (w.ratios >> L) & 1u;
            CHECK(served == has_ratio && calls == (has_ratio ? 1 : 0), "%s L %u PP %d: served %d, %d calls", w.name, L, PP,
                  (int)served, calls);
            if (calls != 1) continue;
            CHECK(lr == (int)L && ppc == want_ppc(w, L, PP), "%s L %u PP %d: <%d, %d>", w.name, L, PP, lr, ppc);
            if (lr >= 0 && lr < 10 && ppc >= 0 && ppc <= 32) seen[lr][ppc] = true;
        }
    // has() itself, over a grid wider than the tables, and the kernels reached
    int has_n = 0, seen_n = 0;
    for (int LR = 0; LR < 10; ++LR)
        for (int PPC = 0; PPC <= 32; ++PPC) {
            const bool want = ((w.ratios >> LR) & 1u) && (PPC == 0 || want_ppc(w, (unsigned)LR, PPC) == PPC);
            CHECK(SHAPES::has(LR, PPC) == want, "%s has(%d, %d)", w.name, LR, PPC);
            has_n += SHAPES::has(LR, PPC);
            seen_n += seen[LR][PPC];
        }
    CHECK(has_n == w.kernels && seen_n == w.kernels, "%s: has %d, reached %d of %d kernels", w.name, has_n, seen_n, w.kernels);
    std::printf("%s: %d kernels\n", w.name, seen_n);
    return cases;
}

int main() {
    static_assert(!UpDot2SummingTile::has(8, 16) && !UpDot2SummingTile::has(8, 32) && UpDot2SummingTile::has(8, 8) &&
                      !UpDot2SummingTile::has(3, 0) && UpDot2Standard::has(8, 16) && !UpDot2Standard::has(8, 32) &&
                      !UpDot2Resampler::has(4, 8) && !UpDot2Standard::has(9, 0) && !UpDot2Standard::has(1, 0),
                  "has() is a constant expression");
    long cases = sweep<UpDot2Standard>(kStandard);
    cases += sweep<UpDot2Resampler>(kResampler);
    cases += sweep<UpDot2SummingTile>(kSumming);
    std::printf("%ld cases, %ld failures\n", cases, fails);
    return fails ? 1 : 0;
}
