// k_gauss.hip -- K1: fused value remap + separable Gaussian x0.3 downsample (gfx950).
//
// Replaces the prologue remap (LSD/myLSD.cpp:135-142) and GaussianSampler (LSD/myLSD.cpp:378-484).
// One workgroup produces a 32x24 tile (TW x TH) of the scaled image: the (reflected, remapped) u8 source
// window is staged in LDS with coalesced row-major loads, the x-pass writes an fp64 LDS strip,
// the y-pass reads it back column-wise.  The reference's aux[H][w] image never exists in HBM.
//
// Bit-exactness: same taps (computed on the host with the host libm), same accumulation order
// (newVal += pix * ker[i], i ascending), fp64, no FMA contraction (-ffp-contract=off).
#include "lsd_internal.h"
#include "k1_lds.h"
#include "k1_stage.h"
#include <algorithm>

namespace lsdhip {

// Output tile (k1_lds.h says why 32 x 24).
constexpr int TW = kK1TileW, TH = kK1TileH, NT = 256;

// centre_of(x) = (int)floor(x / sca + 0.5) (myLSD.cpp:428 / :460) comes from a table the host fills with exactly that expression
// (lsd_ctx.hip: ensure_tables): an fp64 division per use was a fifth of this kernel's vector instructions.

// HS > 0: the tap count is a compile-time constant (17 for the reference's sca = 0.3, sig = 0.6): the x-pass keeps its
// column's taps in registers and both passes are fully unrolled.  HS == 0: any tap count.
template <int HS>
__global__ __launch_bounds__(NT) void k_gauss(const uint8_t* __restrict__ in, double* __restrict__ out,
                                              const double* __restrict__ taps_g, const int* __restrict__ centre_of, int W, int H, int w, int h, int gp,
                                              int tapR, int IWp, int IHmax, unsigned gx, unsigned gy, unsigned tiles,
                                              uint8_t* __restrict__ clr, uint32_t keep_all) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int hSize = HS > 0 ? HS : 2 * tapR + 1;
    double* aux = reinterpret_cast<double*>(smem);                // [IHmax][TW]
    double* taps = aux + (size_t)IHmax * TW;                      // [3][hSize]
    uint8_t* tile = reinterpret_cast<uint8_t*>(taps + 3 * hSize); // [IHmax][IWp]

    const int tid = threadIdx.x;
    // Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one, each XCD has its own L2): the tiles are numbered
    // such that one XCD walks a contiguous eighth of the batch, so the 15-pixel halo a tile shares with its neighbours comes out
    // of the L2 the neighbouring tile has just filled.
    const unsigned per = (tiles + 7u) >> 3;
    const unsigned t = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (t >= tiles) return;
    const unsigned bx = t % gx, tq = t / gx, by = tq % gy;
    const int X0 = (int)bx * TW, Y0 = (int)by * TH;
    const size_t img = tq / gy;
    const uint8_t* src = in + img * (size_t)W * H;
    double* dst = out + img * (size_t)gp * h;                     // rows padded to gp doubles (128-byte aligned rows for K2)

    if (clr) {
        // lineIm = Mat::zeros (myLSD.cpp:215), fused: this kernel is bound by its fp64 filter and LDS staging, its store path idles, so every
        // tile clears the t-th of its image's `tiles per image` contiguous shares of the raster on the way (16 bytes per lane and store,
        // non-temporal; launch_gauss only passes the raster when its size and address are multiples of 16).  As a kernel of its own the
        // clear took 0.44 ms of the bench step.
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const unsigned tpi = gx * gy, ti = t % tpi;
        const size_t units = ((size_t)W * H) >> 4;
        const size_t a = units * ti / tpi, e = units * (ti + 1) / tpi;
        u32x4* const v = reinterpret_cast<u32x4*>(clr + img * (size_t)W * H);
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (size_t u = a + tid; u < e; u += NT) __builtin_nontemporal_store(z, &v[u]);
    }
    const int Xl = min(X0 + TW - 1, w - 1), Yl = min(Y0 + TH - 1, h - 1);
    const int c0 = centre_of[X0] - tapR, c1 = centre_of[Xl] + tapR;
    const int r0 = centre_of[Y0] - tapR, r1 = centre_of[Yl] + tapR;
    const int IH = r1 - r0 + 1;

    for (int i = tid; i < 3 * hSize; i += NT) taps[i] = taps_g[i];

    // stage the source window (k1_stage.h; window columns start at a0 = c0 rounded down to a multiple of 4)
    const int a0 = c0 - (((c0 % 4) + 4) % 4);
    const uint32_t wany = stage_window(src, tile, W, H, r0, r1, a0, c1, IWp, tid, keep_all);   // has this thread staged anything but zeros?
    // A window of zeros -- free and unknown cells only: 47 % of the bench maps' windows -- gives a tile of +0.0 (every product is +0.0 * tap,
    // every sum +0.0 + +0.0): both passes and their barrier are skipped (K1 2.92 -> 2.59 ms on the bench batch, same bits).  Measured with
    // it and dropped: one word per window row saying which of its words / x-pass sums are non-zero, so that the passes' zero tests
    // read one word instead of 5 words / 17 doubles -- 0.19 ms SLOWER: the kernel is bound by the latency of its staging, not by those tests.
    const int X = tid & (TW - 1);
    const int gX = X0 + X;
    if (!__syncthreads_or((int)(wany != 0u))) {
        if (gX < w)
            for (int Y = tid / TW; Y < TH && Y0 + Y < h; Y += NT / TW) dst[(size_t)(Y0 + Y) * gp + gX] = 0.0;
        return;
    }
    {
        const int cb = (gX < w ? centre_of[gX] : 0) - tapR - a0;            // first tap's column inside the window
        const double* ker = taps + (gX % 3) * hSize;
        if (gX < w) {
            if constexpr (HS > 0) {
                static_assert(HS == 17, "the x-pass reads 5 words = 17 bytes at any byte offset (k1_stage.h: xpass17)");
                double kr[17];
                #pragma unroll
                for (int i = 0; i < HS; i++) kr[i] = ker[i];
                const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile) + (cb >> 2);
                const uint32_t sh = (uint32_t)(cb & 3);
                const int DWp = IWp >> 2;
                for (int r = tid / TW; r < IH; r += NT / TW) aux[r * TW + X] = xpass17(trow + r * DWp, sh, kr);
            } else {
                for (int r = tid / TW; r < IH; r += NT / TW) {
                    const uint8_t* t = tile + r * IWp + cb;
                    double v = 0;
                    for (int i = 0; i < hSize; i++) v += (double)(int)t[i] * ker[i];
                    aux[r * TW + X] = v;
                }
            }
        }
    }
    __syncthreads();

    // y-pass (myLSD.cpp:452-482): out[Y][X] = sum_i aux[yc-h+i][X] * ker[Y%3][i]
    if (gX < w) {
        for (int Y = tid / TW; Y < TH; Y += NT / TW) {
            const int gY = Y0 + Y;
            if (gY >= h) break;
            const int rb = centre_of[gY] - tapR - r0;
            const double* ker = taps + (gY % 3) * hSize;
            double v = 0;
            if (HS > 0) {
                double a[HS > 0 ? HS : 1];
                uint32_t bits = 0u;                            // (the x-pass writes sums of non-negative terms: +0.0 is the only zero)
                #pragma unroll
                for (int i = 0; i < HS; i++) { a[i] = aux[(rb + i) * TW + X]; bits |= (uint32_t)__double2hiint(a[i]) | (uint32_t)__double2loint(a[i]); }
                if (__ballot(bits != 0u) != 0ull) {                    // (all zeros: the sum is +0.0, as in the x-pass)
                    #pragma unroll
                    for (int i = 0; i < HS; i++) v += a[i] * ker[i];
                }
            } else {
                for (int i = 0; i < hSize; i++) v += aux[(rb + i) * TW + X] * ker[i];
            }
            dst[(size_t)gY * gp + gX] = v;
        }
    }
}

// Observable side effect of the reference: the caller's image is rewritten in place (myLSD.cpp:135-142): 1 -> 255, 255 -> 0 for y >= 1,
// x >= 1.  16 bytes per lane where the rows are whole 16-byte units (the byte masks of the staging above, four words at a time), and a
// unit is written back only if it changes -- free space is most of an occupancy map, so most units are only read: 512 maps of 2048^2
// 3.2 -> see DESIGN.md section 5 (one byte per thread with a 64-bit division each before).
__global__ __launch_bounds__(256) void k_remap_inplace16(uint8_t* __restrict__ img, uint32_t W, uint32_t H, size_t units) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4* const v = reinterpret_cast<u32x4*>(img);
    const uint32_t upr = W >> 4;                                  // units per row
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += stride) {
        const u32x4 x = v[u];
        if ((x.x | x.y | x.z | x.w) == 0u) continue;              // free space: nothing to rewrite
        const uint32_t row = (uint32_t)(u / upr), col = (uint32_t)(u - (size_t)row * upr);
        if (row % H == 0u) continue;                              // row 0 of an image keeps its raw values (Q2)
        u32x4 r;
        r.x = remap4(x.x, col == 0u ? 0xffu : 0u);            // ... and so does column 0
        r.y = remap4(x.y, 0u); r.z = remap4(x.z, 0u); r.w = remap4(x.w, 0u);
        if ((r.x ^ x.x) | (r.y ^ x.y) | (r.z ^ x.z) | (r.w ^ x.w)) v[u] = r;
    }
}
__global__ __launch_bounds__(256) void k_remap_inplace(uint8_t* __restrict__ img, int W, int H, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t per = (size_t)W * H;
    for (; i < total; i += stride) {
        const size_t p = i % per;
        const int y = (int)(p / W), x = (int)(p % W);
        if (y >= 1 && x >= 1) {
            uint8_t v = img[i];
            if (v == 1) img[i] = 255; else if (v == 255) img[i] = 0;
        }
    }
}

// clr: lineIm to be cleared on the way (null: none; the caller has checked that every image's raster is a whole number of 16-byte words)
// remapped: the source holds the values the remap has left already (lsd_debug_fetch after a write-back): staged as they are
static auto gauss_kernel(const Geom& g) { return 2 * g.tapR + 1 == 17 ? k_gauss<17> : k_gauss<0>; }

// Before the first enqueue of a call: a window above 64 KiB needs the kernel's dynamic-LDS limit raised (make_geom has checked the size
// against the device's limit).  An error here leaves nothing queued.
hipError_t prepare_gauss(const Geom& g) {
    const K1Lds L = k1_lds(g.sca, g.tapR);
    if (L.bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(gauss_kernel(g)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes);
}

void launch_gauss(const Geom& g, const Buffers& b, int n, uint8_t* clr, bool remapped, hipStream_t s) {
    const K1Lds L = k1_lds(g.sca, g.tapR);
    const unsigned gx = (g.w + TW - 1) / TW, gy = (g.h + TH - 1) / TH, tiles = gx * gy * (unsigned)n;
    hipLaunchKernelGGL(gauss_kernel(g), dim3(((tiles + 7u) >> 3) * 8u), dim3(NT), L.bytes, s, b.in, b.gauss, b.taps, b.centres, g.W, g.H, g.w, g.h, g.gp,
                       g.tapR, L.IWp, L.IHmax, gx, gy, tiles, clr, remapped ? 0xffffffffu : 0u);
}

void launch_remap_writeback(const Geom& g, const Buffers& b, int n, hipStream_t s) {
    if (!b.in_rw) return;
    const size_t total = (size_t)n * g.W * g.H;
    if ((g.W & 15) == 0 && (reinterpret_cast<uintptr_t>(b.in_rw) & 15) == 0) {      // rows of whole 16-byte units
        const size_t units = total >> 4;
        const int blocks = (int)std::min<size_t>((units + 255) / 256, 16384);
        hipLaunchKernelGGL(k_remap_inplace16, dim3(blocks), dim3(256), 0, s, b.in_rw, (uint32_t)g.W, (uint32_t)g.H, units);
        return;
    }
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_remap_inplace, dim3(blocks), dim3(256), 0, s, b.in_rw, g.W, g.H, total);
}

}  // namespace lsdhip
