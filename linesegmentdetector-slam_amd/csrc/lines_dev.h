// lines_dev.h -- K5's body: one image's accepted rectangles -> structLinesInfo records + lineIm raster (gfx950).
//
// Replaces myLSD.cpp:280-368 (and sind/cosd/atand, LSD/baseFunc.cpp:6-16).  One wavefront per line (strided by the caller's number of
// wavefronts); lanes walk the samples of the longer axis.  lineIm has been cleared earlier on the same stream; marking 255 is
// idempotent so store order is free.  Shared by k_lines (k_lines.hip: one workgroup per image, behind the region stage) and by the region
// stage itself (k_region.hip: the workgroup that has just finished an image writes its lines): one text, the same expressions in the
// same order, so the records are the same bits whichever of the two runs.
#pragma once
#include "lsd_internal.h"
#include "devmath.h"

namespace lsdhip {

// A record word as the region stage's wavefronts left it: a plain vector load.  (The line number is the same in every lane, and a load the
// compiler can prove uniform and unclobbered goes through the scalar cache, which the vector stores of the workgroup's other wavefronts
// -- and of the workgroups that share the cache, whose images' records may lie in the same cache line -- do not update.)
__device__ __forceinline__ double rec_word(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// `count`: the image's line count as the region stage left it (more than max_lines: clamped, the overflow is the host's to report; -1, an
// image given up: no lines); rs / out / im: this image's scaled records, line array and raster (im may be null).
__device__ __forceinline__ void lines_of_image(const double* rs, int count, lsd_line* __restrict__ out, uint8_t* __restrict__ im,
                                               int max_lines, int W, int H, int wave, int lane, int nwaves) {
    int n = count;
    if (n > max_lines) n = max_lines;
    for (int i = wave; i < n; i += nwaves) {
        const double x1 = rec_word(rs + i * 4 + 0), y1 = rec_word(rs + i * 4 + 1), x2 = rec_word(rs + i * 4 + 2), y2 = rec_word(rs + i * 4 + 3);
        const double k = (y2 - y1) / (x2 - x1);                                    // :289
        double ang = atan_g(k) * 180.0 / kPi;                                        // atand, baseFunc.cpp:14-16
        int orient = 1;
        if (ang < 0) { ang += 180; orient = -1; }                                  // :292-295
        int xLow, xHigh, yLow, yHigh;
        if (x1 > x2) { xLow = cvt_x86(floor(x2)); xHigh = cvt_x86(ceil(x1)); }     // :298-305
        else         { xLow = cvt_x86(floor(x1)); xHigh = cvt_x86(ceil(x2)); }
        if (y1 > y2) { yLow = cvt_x86(floor(y2)); yHigh = cvt_x86(ceil(y1)); }     // :306-313
        else         { yLow = cvt_x86(floor(y1)); yHigh = cvt_x86(ceil(y2)); }
        const double xRang = fabs(x2 - x1), yRang = fabs(y2 - y1);
        const int xx_len = xHigh - xLow + 1, yy_len = yHigh - yLow + 1;
        if (im) {
            // Q10: only the sampled part of the reference's marking loop is defined behaviour
            if (xRang > yRang) {                                                   // :319-330
                for (int j = lane; j < xx_len; j += 64) {
                    const int xx = j + xLow;
                    const int yy = cvt_x86(round((xx - x1) * k + y1));
                    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                    if (xx != 0 && yy != 0) im[(size_t)yy * W + xx] = 255;        // :346
                }
            } else {                                                               // :331-342
                for (int j = lane; j < yy_len; j += 64) {
                    const int yy = j + yLow;
                    const int xx = cvt_x86(round((yy - y1) / k + x1));
                    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                    if (xx != 0 && yy != 0) im[(size_t)yy * W + xx] = 255;        // :352
                }
            }
        }
        if (lane == 0) {
            lsd_line L;
            L.k = k;
            L.b = (y1 + y2) / 2.0 - k * (x1 + x2) / 2.0;                           // :359
            sincos_g(ang / 180.0 * kPi, L.dy, L.dx);                               // sind / cosd
            L.x1 = x1; L.y1 = y1; L.x2 = x2; L.y2 = y2;
            const double ey = y2 - y1, ex = x2 - x1;
            L.len = sqrt(ey * ey + ex * ex);                                       // :366
            L.orient = orient;
            out[i] = L;
            reinterpret_cast<uint32_t*>(&out[i])[19] = 0u;      // the tail padding of structLinesInfo: defined bytes (records are compared and moved as words)
        }
    }
}

}  // namespace lsdhip
