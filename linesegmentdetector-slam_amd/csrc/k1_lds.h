// k1_lds.h -- the LDS a workgroup of K1 (k_gauss.hip) needs, as a function of the scale and the tap radius alone.
//
// Shared by launch_gauss (which sizes the launch by it) and make_geom (which refuses a parameter set whose window does not fit the
// device's LDS before anything is enqueued).  Plain C++, no HIP: tests/k1_lds_host.cpp compiles it with the host compiler and pins
// the formula (tests/test_abi.py).
#pragma once
#include <math.h>
#include <stddef.h>

namespace lsdhip {

// K1's output tile: 32 wide, 24 high.  The height sets the LDS a workgroup needs (the x-pass sums of the window's rows: 38 KB at 24, 49 KB
// at 32, 27 KB at 16) against the rows of the window that neighbouring tiles compute twice; the kernel is bound by the latency of its
// staging, so workgroups per CU count: 32 -> 24 rows (four workgroups per CU instead of three) 2.58 -> 2.35 ms on the bench batch, 16
// rows (five) 2.83 (profiles/r06g_k1_tile_heights.log; same bits).
#ifndef LSD_K1_TH
#define LSD_K1_TH 24
#endif
constexpr int kK1TileW = 32, kK1TileH = LSD_K1_TH;

struct K1Lds {
    int IWp;        // row pitch (bytes) of the staged u8 window
    int IHmax;      // rows of the largest window a tile can have
    size_t bytes;   // dynamic LDS of the launch: x-pass sums [IHmax][TW] fp64 + taps [3][hSize] fp64 + window [IHmax][IWp] u8
};

inline K1Lds k1_lds(double sca, int tapR) {
    K1Lds r;
    const int span = (int)floor((kK1TileW - 1) / sca) + 2;       // bound on centre(X0+31) - centre(X0) + 1
    const int IWmax = span + 2 * tapR + 1;
    r.IWp = ((IWmax + 3) & ~3) + 8;                               // + the alignment slack of the word-wise staging and of the x-pass's 5-word reads
    if (((r.IWp >> 2) & 1) == 0) r.IWp += 4;                      // odd pitch in 32-bit words: consecutive rows start in different LDS banks
    r.IHmax = (int)floor((kK1TileH - 1) / sca) + 2 + 2 * tapR + 1;   // (as IWmax, for the tile's height)
    const int hSize = 2 * tapR + 1;
    r.bytes = (size_t)r.IHmax * kK1TileW * sizeof(double) + 3 * (size_t)hSize * sizeof(double) + (size_t)r.IHmax * r.IWp;
    return r;
}

}  // namespace lsdhip
