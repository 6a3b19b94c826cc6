// up_dot2_dispatch.h -- which instantiations <LR, PPC> of the v_dot2 tile
// (up_dot2_tile, up_dot2_kernels.h) each kernel family has, and the one place
// that turns a call's run-time shape into one of them, for the six launchers
// (upsamp.hip, upmix.hip, modulate.hip, modulate_offset.hip, modulate_sum.hip,
// resample.hip) and the host program that checks it
// (tests/cpp/up_dot2_dispatch_main.cpp).  Plain C++, no HIP types.
//
// LR is the interpolation ratio L; PPC the tap pairs per phase PP = ceil(H / 2)
// as a compile-time constant, or 0 for the kernel that takes them at run time.
// A family is a table of its compiled shapes (PPC > 0) and the ratios it has;
// every ratio it has also has the run-time kernel <LR, 0>.  A call runs
// <L, PP> where that is a compiled shape and <L, 0> otherwise.
#pragma once
#include <type_traits>

namespace srcdsp {

struct UpShape {
    int LR, PPC;
};

template <int N>
constexpr bool up_shape_listed(const UpShape (&shapes)[N], int LR, int PPC) {
    for (int i = 0; i < N; ++i)
        if (shapes[i].LR == LR && shapes[i].PPC == PPC) return true;
    return false;
}

constexpr int kUpDot2MinL = 2, kUpDot2MaxL = 8;  // the tile's ratios

// up_tile_dot2, upmix_tile_dot2, modulate_tile_dot2, modoffset_tile_dot2: 16,
// 32 or 64 taps per phase (L = 4 x 64 / 128 / 256 taps, L = 2 x 32 / 64 / 128,
// L = 8 x 128 / 256)
struct UpDot2Standard {
    static constexpr UpShape kCompiled[] = {{2, 8}, {2, 16}, {2, 32}, {4, 8}, {4, 16}, {4, 32}, {8, 8}, {8, 16}};
    static constexpr bool has(int LR, int PPC) {
        return LR >= kUpDot2MinL && LR <= kUpDot2MaxL && (PPC == 0 || up_shape_listed(kCompiled, LR, PPC));
    }
};

// resample_tile_dot2: the pairs per phase compiled in at the measured shapes
// (128 taps at L = 4 and 8, 64 at L = 2)
struct UpDot2Resampler {
    static constexpr UpShape kCompiled[] = {{2, 16}, {4, 16}, {8, 8}};
    static constexpr bool has(int LR, int PPC) {
        return LR >= kUpDot2MinL && LR <= kUpDot2MaxL && (PPC == 0 || up_shape_listed(kCompiled, LR, PPC));
    }
};

// modsum_tile_dot2: L = 2, 4 or 8.  L = 8 has 16 taps per phase only:
// modsum_tile_dot2<8, 16, *> gave a wrong wire on hardware
// (tests/test_gpu_modulate_sum_sweep.py at 31 and 32 taps per phase, with and
// without staggers; the same with its first pair through the builtin, so not
// the inline v_dot2), where every other instantiation and the run-time kernel
// on the same shapes equal the model.  The cause was not found, so (8, 16) and
// (8, 32) stay out of the table and those calls run the run-time kernel.
struct UpDot2SummingTile {
    static constexpr UpShape kCompiled[] = {{2, 8}, {2, 16}, {2, 32}, {4, 8}, {4, 16}, {4, 32}, {8, 8}};
    static constexpr bool has(int LR, int PPC) {
        return (LR == 2 || LR == 4 || LR == 8) && (PPC == 0 || up_shape_listed(kCompiled, LR, PPC));
    }
};

// the compiled shape (L, PP) of SHAPES' table, from entry I on
template <class SHAPES, int I, class F>
bool up_dot2_compiled(unsigned L, int PP, F &f) {
    if constexpr (I < (int)(sizeof(SHAPES::kCompiled) / sizeof(UpShape))) {
        constexpr UpShape s = SHAPES::kCompiled[I];
        static_assert(s.PPC > 0 && SHAPES::has(s.LR, 0), "a compiled shape of a ratio the family has");
        if (L == (unsigned)s.LR && PP == s.PPC) {
            f(std::integral_constant<int, s.LR>{}, std::integral_constant<int, s.PPC>{});
            return true;
        }
        return up_dot2_compiled<SHAPES, I + 1>(L, PP, f);
    } else {
        return false;
    }
}

// the run-time kernel <L, 0>, from ratio LR on
template <class SHAPES, int LR, class F>
bool up_dot2_runtime(unsigned L, F &f) {
    if constexpr (LR <= kUpDot2MaxL) {
        if constexpr (SHAPES::has(LR, 0)) {
            if (L == (unsigned)LR) {
                f(std::integral_constant<int, LR>{}, std::integral_constant<int, 0>{});
                return true;
            }
        }
        return up_dot2_runtime<SHAPES, LR + 1>(L, f);
    } else {
        return false;
    }
}

// f(integral_constant<int, LR>, integral_constant<int, PPC>), once, with the
// instantiation SHAPES assigns to (L, PP); false and no call where SHAPES has
// no kernel of ratio L.  Only shapes SHAPES::has are instantiated.
template <class SHAPES, class F>
bool up_dot2_dispatch(unsigned L, int PP, F f) {
    return up_dot2_compiled<SHAPES, 0>(L, PP, f) || up_dot2_runtime<SHAPES, kUpDot2MinL>(L, f);
}

}  // namespace srcdsp
