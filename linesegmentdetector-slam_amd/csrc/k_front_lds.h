// k_front_lds.h -- the LDS a workgroup of the fused front end (k_front.hip) needs, as a function of the scale and the tap radius.
//
// The fused kernel takes a K1 tile (k1_lds.h: 32 x 24) plus the row above it and the column left of it through the Gaussian, so its
// window and its x-pass strip are those of a 33 x 25 tile.  Once the y-pass is over both are dead, and the gradient part lives in
// their place: the Gaussian tile, the list counter and the per-wave maxima where the u8 window was, the list of non-zero-gradient
// pixels where the x-pass strip was.  Plain C++, no HIP.
#pragma once
#include <math.h>
#include <stddef.h>
#include "k1_lds.h"

namespace lsdhip {

constexpr int kFrontGW = kK1TileW + 1, kFrontGH = kK1TileH + 1;   // the Gaussian tile with its halo
constexpr int kFrontList = kK1TileW * kK1TileH;                   // list entries: every pixel of a tile may have a non-zero gradient

struct KFrontLds {
    int IWp;           // row pitch (bytes) of the staged u8 window
    int IHmax;         // rows of the largest window a tile can have
    size_t strip;      // bytes of the first region: x-pass sums [IHmax][kFrontGW] fp64, later the list (16 + 4 bytes per entry)
    size_t window;     // bytes of the last region: window [IHmax][IWp] u8, later Gaussian tile + list counter + 4 per-wave maxima
    size_t bytes;      // dynamic LDS of the launch: strip + taps [3][hSize] fp64 + window
};

inline KFrontLds k_front_lds(double sca, int tapR) {
    KFrontLds r;
    const int span = (int)floor(kK1TileW / sca) + 2;              // bound on centre(X0+31) - centre(X0-1) + 1
    const int IWmax = span + 2 * tapR + 1;
    r.IWp = ((IWmax + 3) & ~3) + 8;                               // (the alignment slack and the odd word pitch of k1_lds.h)
    if (((r.IWp >> 2) & 1) == 0) r.IWp += 4;
    r.IHmax = (int)floor(kK1TileH / sca) + 2 + 2 * tapR + 1;
    const int hSize = 2 * tapR + 1;
    const size_t sums = (size_t)r.IHmax * kFrontGW * sizeof(double), list = (size_t)kFrontList * (16 + 4);
    const size_t win = ((size_t)r.IHmax * r.IWp + 7) & ~(size_t)7, post = (size_t)kFrontGW * kFrontGH * sizeof(double) + 8 + 4 * 8;
    r.strip = ((sums > list ? sums : list) + 15) & ~(size_t)15;
    r.window = win > post ? win : post;
    r.bytes = r.strip + 3 * (size_t)hSize * sizeof(double) + r.window;
    return r;
}

}  // namespace lsdhip
