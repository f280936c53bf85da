// k1_stage.h -- what the two front-end kernels share (K1, k_gauss.hip, and the fused front end, k_front.hip): staging of the
// reflected, remapped u8 source window in LDS, and the 17-tap x-pass sum of one window row.  Device code, 256 threads per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsdhip {

__device__ __forceinline__ int reflect_idx(int j, int lim) {  // myLSD.cpp:436-443
    const int dou = 2 * lim;
    while (j < 0) j += dou;
    while (j >= dou) j -= dou;
    if (j >= lim) j = dou - j - 1;
    return j;
}

// bytes == 1 -> 255, bytes == 255 -> 0 (myLSD.cpp:135-142) on the four bytes of a word, except where `keep` has a byte of ones
__device__ __forceinline__ uint32_t remap4(uint32_t x, uint32_t keep) {
    uint32_t t1 = x ^ 0x01010101u, t2 = ~x;                   // zero bytes mark the two cases
    t1 = ~(((t1 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t1 | 0x7f7f7f7fu);   // 0x80 in every byte that was zero
    t2 = ~(((t2 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t2 | 0x7f7f7f7fu);
    const uint32_t m1 = (t1 | (t1 - (t1 >> 7))) & ~keep, m255 = (t2 | (t2 - (t2 >> 7))) & ~keep;   // 0x80 -> 0xff (no multiply)
    return (x | m1) & ~m255;
}

// Stages source rows r0 .. r0 + IH - 1, columns a0 .. c1 (a0 a multiple of 4 in window terms: c0 rounded down) of one image as 32-bit
// words with a row pitch of IWp bytes: every thread first issues all its loads (up to 16 words in flight), then remaps
// (myLSD.cpp:135-142) and stores to LDS.  keep_all: all ones when the source has been remapped already (the remap is not idempotent:
// 1 -> 255 -> 0), else 0.  Returns whether this thread has staged anything but zeros.
__device__ __forceinline__ uint32_t stage_window(const uint8_t* __restrict__ src, uint8_t* tile, int W, int H, int r0, int r1, int a0, int c1,
                                                 int IWp, int tid, uint32_t keep_all) {
    uint32_t wany = 0u;
    const int IH = r1 - r0 + 1;
    // 32 word columns x 8 rows of threads: a thread keeps its word column and walks down the window 8 rows at a time, so the
    // column work (bounds, reflection, "column 0 keeps raw values") is done once and nothing is divided
    const int DW = (c1 - a0 + 4) >> 2;                        // words per window row
    uint32_t* tile32 = reinterpret_cast<uint32_t*>(tile);
    const int DWp = IWp >> 2;
    const int tx = tid & 31, ty = tid >> 5;
    // A window that lies inside the image, off its row 0 and column 0 (which keep their raw values, Q2), with aligned words: nothing
    // is reflected and nothing exempt -- all but the tiles on the border (wave-uniform)
    const bool plain = a0 >= 4 && a0 + 4 * DW <= W && r0 >= 1 && r1 < H && (W & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    if (plain) {
        // whole groups of 8 window rows (one per row of threads) under wave-uniform conditions: a scalar row base plus one 32-bit
        // lane offset; the window's last IH % 8 rows under a lane mask, once
        const int nfull = IH >> 3, tail = IH & 7;
        const uint8_t* const sb = src + (size_t)r0 * W + a0;
        for (int cw = tx; cw < DW; cw += 32) {
            const uint32_t voff = (uint32_t)ty * (uint32_t)W + 4u * (uint32_t)cw;
            uint32_t* const t0 = tile32 + ty * DWp + cw;
            for (int g0 = 0; g0 < nfull; g0 += 16) {
                uint32_t v[16];
                #pragma unroll
                for (int j = 0; j < 16; j++) {
                    v[j] = 0u;
                    if (g0 + j < nfull) v[j] = *reinterpret_cast<const uint32_t*>(sb + (size_t)(g0 + j) * 8u * (size_t)W + voff);
                }
                #pragma unroll
                for (int j = 0; j < 16; j++) {
                    // words of 0 (free) and of 255s (unknown: 0 after the remap) are most of an occupancy map: where a whole wavefront
                    // sees nothing else there is nothing to compute
                    if (g0 + j < nfull) { const uint32_t rm = __ballot(v[j] + 1u > 1u) != 0ull ? remap4(v[j], keep_all) : (keep_all & v[j]); t0[(g0 + j) * 8 * DWp] = rm; wany |= rm; }
                }
            }
            if (ty < tail) { const uint32_t rm = remap4(*reinterpret_cast<const uint32_t*>(sb + (size_t)nfull * 8u * (size_t)W + voff), keep_all); t0[nfull * 8 * DWp] = rm; wany |= rm; }
        }
    } else
    for (int cw = tx; cw < DW; cw += 32) {
        const int gx0 = a0 + 4 * cw;
        const bool fast_col = gx0 >= 0 && gx0 + 3 < W;        // the whole word lies inside the image
        int gxr[4];
        uint32_t colkeep = keep_all;                          // bytes of source column 0: exempt from the remap (Q2)
        #pragma unroll
        for (int k2 = 0; k2 < 4; k2++) {
            gxr[k2] = reflect_idx(gx0 + k2, W);
            if (gxr[k2] == 0) colkeep |= 0xffu << (8 * k2);
        }
        for (int rb = 0; rb < IH; rb += 8 * 16) {
            uint32_t v[16];
            #pragma unroll
            for (int j = 0; j < 16; j++) {
                const int r = rb + ty + 8 * j;
                v[j] = 0u;
                if (r < IH) {
                    const int gy = reflect_idx(r0 + r, H);
                    const size_t off = (size_t)gy * W + gx0;
                    if (fast_col && (off & 3) == 0) v[j] = *reinterpret_cast<const uint32_t*>(src + off);
                    else {
                        const uint8_t* row = src + (size_t)gy * W;
                        v[j] = (uint32_t)row[gxr[0]] | ((uint32_t)row[gxr[1]] << 8) | ((uint32_t)row[gxr[2]] << 16) | ((uint32_t)row[gxr[3]] << 24);
                    }
                }
            }
            #pragma unroll
            for (int j = 0; j < 16; j++) {
                const int r = rb + ty + 8 * j;
                if (r < IH) {
                    // row 0 and column 0 keep their raw values (Q2)
                    const uint32_t x = v[j];
                    const uint32_t rm = x != 0u ? remap4(x, reflect_idx(r0 + r, H) == 0 ? 0xffffffffu : colkeep) : 0u;
                    tile32[r * DWp + cw] = rm; wany |= rm;
                }
            }
        }
    }
    return wany;
}

// The x-pass sum of one window row for 17 taps kept in registers (kr): t4 points at the aligned word that holds the first tap's byte,
// sh is that byte's offset in it.  The 17 window bytes start at any byte offset: read the 5 aligned words that hold them
// (conflict-free: the lanes of a row spread over ~27 banks and the odd row pitch separates the wave's two rows) and shift them into
// place.  Occupancy maps are mostly zeros after the remap (free and unknown cells): where the whole wavefront sees zeros the sum is
// +0.0 exactly (every term is +0.0 * tap = +0.0, and +0.0 + +0.0 = +0.0).
__device__ __forceinline__ double xpass17(const uint32_t* t4, uint32_t sh, const double (&kr)[17]) {
    const uint32_t d0 = t4[0], d1 = t4[1], d2 = t4[2], d3 = t4[3], d4 = t4[4];
    if (__ballot((d0 | d1 | d2 | d3 | d4) != 0u) == 0ull) return 0.0;
    uint32_t wv[5];
    wv[0] = __builtin_amdgcn_alignbyte(d1, d0, sh); wv[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    wv[2] = __builtin_amdgcn_alignbyte(d3, d2, sh); wv[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
    wv[4] = d4 >> (8u * sh);
    double v = 0;
    #pragma unroll
    for (int i = 0; i < 17; i++) v += (double)(int)((wv[i >> 2] >> (8 * (i & 3))) & 0xffu) * kr[i];
    return v;
}

}  // namespace lsdhip
