// resample_index.h -- the index arithmetic of the interpolator -> decimator
// tile (resample_tile_dot2, resample_kernels.h), in one place for the kernel,
// its launcher and the host program that checks it
// (tests/cpp/resample_index_main.cpp).  Plain C++, no HIP types.
//
// A tile is kRsTile inputs j0 = kRsTile * tile .. j0 + kRsTile - 1 of the
// interpolator's virtual stream (history ++ input ++ flush zeros) and the
// L * kRsTile interpolated ("mid") words L j0 .. L (j0 + kRsTile) - 1 they make.
// In LDS the mid words stand behind the interpolator's input planes as one
// plane of entries (re pair, im pair): entry e holds local words 2e and 2e + 1,
// local word a being mid word L j0 - HP + a.  The first HP local words are the
// halo (the mid words before the tile), the next L * kRsTile the tile's own, and
// one spare pair of entries closes the plane (it keeps the next region 16-byte
// aligned; an even-aligned output reads the word behind its own against the
// zero tap c[-1], which for the tile's last word is the spare entry's).
#pragma once

#ifdef __HIPCC__
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace srcdsp {

constexpr int kRsTile = 2048;  // inputs per tile: kUpTile of up_dot2_kernels.h

// halo words staged ahead of a tile's mid words: the N_d - 1 words the first
// output's taps reach back, the word one deeper that the zero tap c[N_d] of
// the last pair of an even N_d (or the low half of an odd-aligned last pair)
// multiplies, rounded up to whole 16-byte entry pairs
RS_HD constexpr int rs_halo_words(int Nd) { return (Nd + 1 + 7) & ~7; }

// tap pairs of the decimator: P_j = (lo c[2j], hi c[2j-1]), j <= N_d / 2; the
// decimator stage walks them four at a time, zero pairs behind the last
RS_HD constexpr int rs_decim_pairs(int Nd) { return Nd / 2 + 1; }
RS_HD constexpr int rs_decim_pairs4(int Nd) { return (rs_decim_pairs(Nd) + 3) & ~3; }

// input samples ahead of j0 whose outputs the halo holds
RS_HD constexpr int rs_halo_inputs(int L, int HP) { return (HP + L - 1) / L; }

// the planes' depth: halo granules (8 samples) staged ahead of j0, for the
// 2 PP samples the PP tap pairs of a phase reach back from the earliest sample
// whose output the halo recomputes
RS_HD constexpr int rs_halo_granules(int PP, int L, int HP) { return (2 * PP + rs_halo_inputs(L, HP) + 7) / 8; }

// dwords of one input plane (4 per granule of 8 samples)
RS_HD constexpr int rs_plane_dwords(int HG) { return 4 * (kRsTile / 8 + HG); }

// entries of the mid plane
RS_HD constexpr int rs_mid_entries(int L, int HP) { return HP / 2 + L * kRsTile / 2 + 2; }

// dynamic LDS of a tile: four input planes, then the mid plane, then the
// decimator's tap pairs
RS_HD constexpr unsigned long rs_planes_bytes(int HG) { return 4ul * 4ul * (unsigned long)rs_plane_dwords(HG); }
RS_HD constexpr unsigned long rs_mid_bytes(int L, int HP) { return 8ul * (unsigned long)rs_mid_entries(L, HP); }
RS_HD constexpr unsigned long rs_smem(int H, int L, int Nd) {
    return rs_planes_bytes(rs_halo_granules((H + 1) / 2, L, rs_halo_words(Nd))) + rs_mid_bytes(L, rs_halo_words(Nd)) +
           8ul * (unsigned long)rs_decim_pairs4(Nd);  // both alignments' pairs
}

// a tile's outputs: every i with L j0 <= i M < L (j0 + kRsTile), below n_out
RS_HD constexpr long rs_out_lo(long tile, int L, int M) { return ((long)L * kRsTile * tile + M - 1) / M; }
RS_HD constexpr long rs_out_hi(long tile, int L, int M, long n_out) {
    return rs_out_lo(tile + 1, L, M) < n_out ? rs_out_lo(tile + 1, L, M) : n_out;
}

// local word of mid word i M, the latest word output i of the tile reads with a
// non-zero tap
RS_HD constexpr int rs_out_word(long i, long tile, int L, int M, int HP) {
    return (int)(i * M - (long)L * kRsTile * tile) + HP;
}
// the entries output i's pairs read: rs_out_entry_lo .. rs_out_entry_hi (local
// words 2 (a/2) and 2 (a/2) + 1 first, either parity of a; the zero pairs that
// fill the last four read on: HP / 2 = rs_decim_pairs4)
RS_HD constexpr int rs_out_entry_hi(int a) { return a >> 1; }
RS_HD constexpr int rs_out_entry_lo(int a, int Nd) { return (a >> 1) - (rs_decim_pairs4(Nd) - 1); }

// halo word h (0 <= h < HP) of a tile >= 1 is mid word L j0 - HP + h (>= 0: L *
// kRsTile > HP): output phase rs_halo_phase of the input sample staged at
// rs_halo_sample (counted from the planes' first sample, j0 - 8 HG)
RS_HD constexpr long rs_halo_mid(int h, long tile, int L, int HP) { return (long)L * kRsTile * tile - HP + h; }
RS_HD constexpr int rs_halo_phase(int h, long tile, int L, int HP) { return (int)(rs_halo_mid(h, tile, L, HP) % L); }
RS_HD constexpr int rs_halo_sample(int h, long tile, int L, int HP, int HG) {
    return (int)(rs_halo_mid(h, tile, L, HP) / L - (long)kRsTile * tile) + 8 * HG;
}

}  // namespace srcdsp
