// resample_index_main.cpp -- the index arithmetic of the interpolator ->
// decimator tile (srcdsp_amd/csrc/resample_index.h) checked on the host, built
// with -fsanitize=address,undefined by tests/test_resample_capi.py.  The tile's
// own reads are replayed on a plane of the size the launcher allocates, so an
// index outside it is also an ASan finding.
//
// For every L = 2..8, M = 1..8, N_d in {2, 31, 96, 255, cap}, H in {4, 16, 32}
// and call length of tests/test_gpu_resample.py (those with L n % M == 0):
//   1. the tiles' output ranges partition [0, n_out) in order;
//   2. every halo word of a tile >= 1 maps to an (input, phase) whose tap pairs
//      read inside the staged input planes;
//   3. the entries the decimator stage reads for each output, and the words of
//      the new history, lie inside halo ++ tile (++ the spare entry pair).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../srcdsp_amd/csrc/resample_index.h"

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

int main(int argc, char **argv) {
    const int cap = argc > 1 ? std::atoi(argv[1]) : 1024;
    const int Nds[] = {2, 31, 96, 255, cap};
    const int Hs[] = {4, 16, 32};
    const long calls[] = {4100, 256, 8, 20, 12, 2048, 2560, 9000, 1, 2049, 4096};
    long cases = 0;
    for (int L = 2; L <= 8; ++L)
        for (int M = 1; M <= 8; ++M)
            for (int Nd : Nds)
                for (int H : Hs) {
                    const int PP = (H + 1) / 2, HP = rs_halo_words(Nd), HG = rs_halo_granules(PP, L, HP);
                    const int PDW = rs_plane_dwords(HG), ME = rs_mid_entries(L, HP), J = rs_decim_pairs4(Nd);
                    CHECK(HP % 8 == 0 && HP >= Nd + 1, "HP %d Nd %d", HP, Nd);
                    CHECK(rs_planes_bytes(HG) % 16 == 0, "planes %lu", rs_planes_bytes(HG));
                    CHECK(rs_smem(H, L, Nd) == rs_planes_bytes(HG) + 8ul * ME + 8ul * J && rs_mid_bytes(L, HP) % 16 == 0 &&
                              J % 4 == 0 && J >= Nd / 2 + 1 && rs_smem(H, L, Nd) <= 160 * 1024,
                          "smem %lu", rs_smem(H, L, Nd));
                    std::vector<unsigned> plane((size_t)PDW, 1u);         // one input plane
                    std::vector<unsigned long long> mid((size_t)ME, 1u);  // the mid plane's entries
                    // 2. the halo of a tile >= 1 (the same for every such tile but for j0)
                    for (long tile = 1; tile <= 4; tile += 3)
                        for (int h = 0; h < HP; ++h) {
                            const int o = rs_halo_phase(h, tile, L, HP), jr = rs_halo_sample(h, tile, L, HP, HG);
                            CHECK(o >= 0 && o < L && jr >= 0 && jr < 8 * HG, "L %d Nd %d H %d h %d: o %d jr %d", L, Nd, H,
                                  h, o, jr);
                            // mid word L j0 - HP + h is phase o of input j0 - 8 HG + jr
                            CHECK(rs_halo_mid(h, tile, L, HP) == ((long)kRsTile * tile - 8 * HG + jr) * L + o, "h %d", h);
                            const int d0 = (jr & 1) ? (jr >> 1) : (jr >> 1) - 1;  // pair 0's dword in plane E / O
                            CHECK(d0 - (PP - 1) >= 0 && d0 < PDW, "L %d Nd %d H %d h %d: dwords %d..%d of %d", L, Nd, H, h,
                                  d0 - (PP - 1), d0, PDW);
                            if (d0 - (PP - 1) >= 0 && d0 < PDW)
                                for (int p = 0; p < PP; ++p) fails += plane[(size_t)(d0 - p)] != 1u;
                        }
                    for (long n_total : calls) {
                        const long n_mid = (long)L * n_total;
                        if (n_mid % M) continue;
                        ++cases;
                        const long n_out = n_mid / M, tiles = (n_total + kRsTile - 1) / kRsTile;
                        long next = 0;
                        for (long tile = 0; tile < tiles; ++tile) {
                            const long lo = rs_out_lo(tile, L, M), hi = rs_out_hi(tile, L, M, n_out);
                            // 1. in order, no gap, no overlap
                            CHECK(lo == next && hi >= lo, "L %d M %d n %ld tile %ld: [%ld, %ld) after %ld", L, M, n_total,
                                  tile, lo, hi, next);
                            next = hi;
                            const long m0 = (long)L * kRsTile * tile;
                            for (long i = lo; i < hi; ++i) {
                                // 3. the output's own word is the tile's, its taps reach into the halo at most
                                const int a = rs_out_word(i, tile, L, M, HP);
                                CHECK(i * M >= m0 && i * M < m0 + (long)L * kRsTile && a - (Nd - 1) >= HP - (Nd - 1),
                                      "L %d M %d tile %ld i %ld", L, M, tile, i);
                                const int e_hi = rs_out_entry_hi(a), e_lo = rs_out_entry_lo(a, Nd);
                                CHECK(e_lo >= 0 && e_hi < ME && e_hi - e_lo <= J, "L %d M %d Nd %d i %ld: entries %d..%d of %d",
                                      L, M, Nd, i, e_lo, e_hi, ME);
                                if (e_lo >= 0 && e_hi < ME) fails += mid[(size_t)e_lo] != 1u || mid[(size_t)e_hi] != 1u;
                            }
                        }
                        CHECK(next == n_out, "L %d M %d n %ld: %ld of %ld outputs", L, M, n_total, next, n_out);
                        // the new history: the last N_d - 1 mid words, read by the last tile
                        const long m0 = (long)L * kRsTile * (tiles - 1);
                        const long first = n_mid - (Nd - 1) - m0 + HP;
                        CHECK(first >= 0 && (first + Nd - 2) / 2 < ME - 2 + 1, "L %d Nd %d n %ld: history words from %ld", L,
                              Nd, n_total, first);
                        if (first >= 0 && Nd > 1) fails += mid[(size_t)((first + Nd - 2) >> 1)] != 1u;
                    }
                }
    // the launcher's dynamic LDS at its worst shape: L = 8, 4096 interpolator taps (H = 512), N_d at the cap
    std::printf("smem L=8 H=512 Nd=%d: %lu\n", cap, rs_smem(512, 8, cap));
    std::printf("%ld cases, %ld failures\n", cases, fails);
    return fails ? 1 : 0;
}
