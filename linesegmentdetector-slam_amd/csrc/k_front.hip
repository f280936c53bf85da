// k_front.hip -- the fused front end: K1 (value remap + separable Gaussian x0.3 downsample) and K2 (gradient magnitude, level-line
// angle, threshold map, per-image max) on one tile, for the reference's 17 taps (gfx950).
//
// The Gaussian image has one reader, the 2x2 stencil of the gradient pass (myLSD.cpp:152-174).  Run as two kernels it is written to
// HBM as fp64 and read back (8 B each way per scaled pixel: 3.1 GB of the bench step); here it lives in LDS.  One workgroup takes a
// K1 tile (32 x 24) through staging, remap, x-pass and y-pass exactly as k_gauss<17> does -- same taps, same ascending accumulation,
// fp64, no contraction -- and computes the Gaussian row above the tile and the column left of it as well, as neighbouring tiles
// already recompute the window rows they share: the same expressions on the same inputs, so the halo equals the neighbour's values
// bit for bit.  The (TW+1) x (TH+1) Gaussian tile goes where the staged u8 window was, and the three phases of K2 (k_grad.hip) run on it:
//   1  the dense part (grad_px.h: grad_pixel), three pixels per thread; magnitudes stored; the non-zero-gradient pixels go into a list
//      in LDS, where the x-pass strip was.  The list has an entry for every pixel of the tile: it never has to be flushed half way.
//   2  the list, all 256 threads busy: angle, near-tie count, (sin, cos) where the pixel stays growable;
//   3  angle map and packed pixel words, whole rows.
// k_gauss / k_gradient stay as they are for every other tap count, for lsd_set_stop_after(LSD_STAGE_GAUSS) and for the seed trace.
#include "lsd_internal.h"
#include "k_front_lds.h"
#include "k1_stage.h"
#include "grad_px.h"

namespace lsdhip {

constexpr int TW = kK1TileW, TH = kK1TileH, NT = 256;
constexpr int GW = kFrontGW, GH = kFrontGH;               // the Gaussian tile with its halo: Gt[0][.] is row Y0 - 1, Gt[.][0] column X0 - 1
constexpr int HS = 17, TAPR = 8;
constexpr int PPT = TW * TH / NT;                         // pixels per thread of the gradient part
static_assert(TW == 32 && TW * TH % NT == 0, "a thread keeps its column and walks down the tile NT / TW rows at a time");

// Four workgroups per CU (four wavefronts per SIMD, 128 registers), as K1: the kernel is bound by the latency of its staging.
__global__ __launch_bounds__(NT, 4) void k_front(const uint8_t* __restrict__ in, double* __restrict__ mag, double* __restrict__ deg,
                                                 double2* __restrict__ sc, uint32_t* __restrict__ pw, unsigned long long* __restrict__ maxbits,
                                                 int32_t* __restrict__ ties, const double* __restrict__ taps_g, const int* __restrict__ centre_of,
                                                 int W, int H, int w, int h, double gradThre, int IWp, unsigned strip_bytes, unsigned gx,
                                                 unsigned gy, unsigned tiles, uint8_t* __restrict__ clr) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* aux = reinterpret_cast<double*>(smem);                          // [IH][GW] x-pass sums, column 0 = source of Gt[.][0]
    double* taps = reinterpret_cast<double*>(smem + strip_bytes);           // [3][HS]
    uint8_t* tile = reinterpret_cast<uint8_t*>(taps + 3 * HS);              // [IH][IWp]
    // ... and once they are dead (k_front_lds.h):
    double* Gt = reinterpret_cast<double*>(tile);                           // [GH][GW]
    int* l_cnt = reinterpret_cast<int*>(Gt + GW * GH);                      // entries in the list
    unsigned long long* l_max = reinterpret_cast<unsigned long long*>(l_cnt + 2);   // [4] per-wave maxima
    double2* l_g = reinterpret_cast<double2*>(smem);                        // [kFrontList] in: (gradX, gradY) of the listed pixel; out: (angle, -)
    uint32_t* l_px = reinterpret_cast<uint32_t*>(l_g + kFrontList);         // [kFrontList] (tile-local pixel index << 1) | growable

    const int tid = threadIdx.x;
    // (the tile numbering, the fused lineIm clear and the empty-window test are K1's: k_gauss.hip says why)
    const unsigned per = (tiles + 7u) >> 3;
    const unsigned t = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (t >= tiles) return;
    const unsigned bx = t % gx, tq = t / gx, by = tq % gy;
    const int X0 = (int)bx * TW, Y0 = (int)by * TH;
    const size_t img = tq / gy;
    const uint8_t* src = in + img * (size_t)W * H;
    const size_t base = img * (size_t)w * h;

    if (clr) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const unsigned tpi = gx * gy, ti = t % tpi;
        const size_t units = ((size_t)W * H) >> 4;
        const size_t a = units * ti / tpi, e = units * (ti + 1) / tpi;
        u32x4* const v = reinterpret_cast<u32x4*>(clr + img * (size_t)W * H);
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (size_t u = a + tid; u < e; u += NT) __builtin_nontemporal_store(z, &v[u]);
    }
    // the window of the tile and its halo: scaled columns max(X0 - 1, 0) .. Xl, rows max(Y0 - 1, 0) .. Yl (row 0 and column 0 of the
    // image have no gradient, Q3: no halo there)
    const int Xf = max(X0 - 1, 0), Yf = max(Y0 - 1, 0);
    const int Xl = min(X0 + TW - 1, w - 1), Yl = min(Y0 + TH - 1, h - 1);
    const int c0 = centre_of[Xf] - TAPR, c1 = centre_of[Xl] + TAPR;
    const int r0 = centre_of[Yf] - TAPR, r1 = centre_of[Yl] + TAPR;
    const int IH = r1 - r0 + 1;

    for (int i = tid; i < 3 * HS; i += NT) taps[i] = taps_g[i];

    const int a0 = c0 - (((c0 % 4) + 4) % 4);
    const uint32_t wany = stage_window(src, tile, W, H, r0, r1, a0, c1, IWp, tid, 0u);

    // this thread's pixels: column X of the tile, rows Yt, Yt + 8, Yt + 16
    const int X = tid & (TW - 1), Yt = tid / TW;
    const int gX = X0 + X;
    if (!__syncthreads_or((int)(wany != 0u))) {
        // The extended window holds only zeros (free and unknown cells): the Gaussian tile and its halo are +0.0, so every pixel's
        // result is a constant -- mag = +0.0, deg = 0.0, pw = pack(0.0, gradThre > 0 ? 1 : 0), no list entry, no maximum, no tie.  The
        // constants come out of the general path's own expressions on zeros (the compiler folds them), so that a parameter set with
        // gradThre <= 0 (every zero-gradient pixel growable, (sin, cos) = (0, 1) stored) gets what K2 gives it.
        if (gX < w) {
            #pragma unroll
            for (int k = 0; k < PPT; k++) {
                const int gY = Y0 + Yt + k * (NT / TW);
                if (gY >= h) break;
                const GradPx px = grad_pixel(0.0, 0.0, 0.0, 0.0, gX >= 1 && gY >= 1, gradThre);
                const size_t p = base + (size_t)gY * w + gX;
                mag[p] = px.m;
                if (!px.heavy && px.u == 0) sc[p] = make_double2(0.0, 1.0);
                deg[p] = px.d;
                pw[p] = pack_pw(px.d, px.u);
            }
        }
        return;
    }
    // x-pass (myLSD.cpp:419-450): the tile's 32 columns as in K1 (a thread keeps its column's taps in registers), then the halo
    // column, one window row per thread
    const int DWp = IWp >> 2;
    if (gX < w) {
        const int cb = centre_of[gX] - TAPR - a0;                            // first tap's column inside the window
        const double* ker = taps + (gX % 3) * HS;
        double kr[HS];
        #pragma unroll
        for (int i = 0; i < HS; i++) kr[i] = ker[i];
        const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile) + (cb >> 2);
        const uint32_t sh = (uint32_t)(cb & 3);
        for (int r = Yt; r < IH; r += NT / TW) aux[r * GW + 1 + X] = xpass17(trow + r * DWp, sh, kr);
    }
    if (X0 >= 1 && tid < IH) {
        const int cb = centre_of[X0 - 1] - TAPR - a0;
        const double* ker = taps + ((X0 - 1) % 3) * HS;
        double kr[HS];
        #pragma unroll
        for (int i = 0; i < HS; i++) kr[i] = ker[i];
        const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile) + (cb >> 2);
        for (int r = tid; r < IH; r += NT) aux[r * GW] = xpass17(trow + r * DWp, (uint32_t)(cb & 3), kr);
    }
    __syncthreads();
    if (tid == 0) *l_cnt = 0;                                               // (the window is dead from here on)

    // y-pass (myLSD.cpp:452-482) into the Gaussian tile: Gt[Yh][Xh] = G[Y0 - 1 + Yh][X0 - 1 + Xh]
    for (int idx = tid; idx < GW * GH; idx += NT) {
        const int Yh = idx / GW, Xh = idx - Yh * GW;
        const int gYh = Y0 - 1 + Yh, gXh = X0 - 1 + Xh;
        const bool ok = gYh >= 0 && gYh < h && gXh >= 0 && gXh < w;
        double v = 0;
        if (ok) {
            const int rb = centre_of[gYh] - TAPR - r0;
            const double* ker = taps + (gYh % 3) * HS;
            double a[HS];
            uint32_t bits = 0u;                                // (the x-pass writes sums of non-negative terms: +0.0 is the only zero)
            #pragma unroll
            for (int i = 0; i < HS; i++) { a[i] = aux[(rb + i) * GW + Xh]; bits |= (uint32_t)__double2hiint(a[i]) | (uint32_t)__double2loint(a[i]); }
            if (__ballot(bits != 0u) != 0ull) {                // (all zeros: the sum is +0.0, as in the x-pass)
                #pragma unroll
                for (int i = 0; i < HS; i++) v += a[i] * ker[i];
            }
        }
        Gt[idx] = v;                                           // (outside the image: never used, +0.0 for definiteness)
    }
    __syncthreads();

    // phase 1 (the x-pass strip is dead from here on: the list takes its place)
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long ltmask = (1ull << lane) - 1ull;
    double mx = 0;
    double rowD[PPT];                                          // angle of this thread's k-th pixel ...
    uint32_t rowU[PPT];                                        // ... its usedMap code ...
    int rowSlot[PPT];                                          // ... and, while the angle is still to come, its list slot (else -1)
    #pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int Y = Yt + k * (NT / TW), gY = Y0 + Y;
        const bool valid = gX < w && gY < h;
        const double* g1 = Gt + (Y + 1) * GW + X;              // A = G[y][x], B = G[y][x-1], C = G[y-1][x], D = G[y-1][x-1]
        const GradPx px = grad_pixel(g1[1], g1[0], g1[1 - GW], g1[-GW], valid && gX >= 1 && gY >= 1, gradThre);
        if (valid) {
            const size_t p = base + (size_t)gY * w + gX;
            mag[p] = px.m;
            if (!px.heavy && px.u == 0) sc[p] = make_double2(0.0, 1.0);   // row 0 / col 0: angle 0 exactly, growable (Q3)
        }
        rowD[k] = px.d; rowU[k] = px.u; rowSlot[k] = -1;
        const unsigned long long hm = __ballot(px.heavy);
        if (hm != 0ull) {                                      // (wave-uniform) one LDS atomic per wavefront reserves its entries
            int b0 = 0;
            if (lane == 0) b0 = atomicAdd(l_cnt, __builtin_popcountll(hm));
            b0 = __builtin_amdgcn_readfirstlane(b0);
            if (px.heavy) {
                const int slot = b0 + __builtin_popcountll(hm & ltmask);
                l_px[slot] = ((uint32_t)(Y * TW + X) << 1) | (px.u == 0 ? 1u : 0u);
                l_g[slot] = make_double2(px.gradX, px.gradY);
                rowSlot[k] = slot;
            }
        }
        mx = fmax(mx, px.m);
    }
    // per-image max (myLSD.cpp:167-168): non-negative doubles order like their bit patterns; one atomic per tile
    {
        unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(bits, off);
            bits = o > bits ? o : bits;
        }
        if (lane == 0) l_max[wave] = bits;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long bits = l_max[0];
        #pragma unroll
        for (int i = 1; i < NT / 64; i++) bits = l_max[i] > bits ? l_max[i] : bits;
        if (bits != 0ull) atomicMax(&maxbits[img], bits);
    }

    // phase 2: level-line angle (+ sin/cos where the pixel stays growable) of the listed pixels
    const int cnt = *l_cnt;
    for (int i = tid; i < cnt; i += NT) {
        const uint32_t e = l_px[i];
        const double2 gr = l_g[i];
        const double d = grad_angle(gr.x, gr.y, &ties[img]);   // :169-171
        l_g[i] = make_double2(d, 0.0);
        if (e & 1u) {
            const int lt = (int)(e >> 1);
            sc[base + (size_t)(Y0 + lt / TW) * w + (X0 + lt % TW)] = grad_sincos(d);
        }
    }
    __syncthreads();

    // phase 3: degMap and the packed pixel words, whole rows
    if (gX < w) {
        #pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int gY = Y0 + Yt + k * (NT / TW);
            if (gY < h) {
                const double d = rowSlot[k] >= 0 ? l_g[rowSlot[k]].x : rowD[k];
                const size_t p = base + (size_t)gY * w + gX;
                deg[p] = d;
                pw[p] = pack_pw(d, rowU[k]);
            }
        }
    }
}

bool front_fits(const Geom& g, size_t max_lds) {
    if (2 * g.tapR + 1 != HS) return false;
    const size_t need = k_front_lds(g.sca, g.tapR).bytes;
    return need <= 64 * 1024 && need <= max_lds;                // (within the default dynamic-LDS limit: no attribute to raise)
}

void launch_front(const Geom& g, const Buffers& b, int n, uint8_t* clr, hipStream_t s) {
    const KFrontLds L = k_front_lds(g.sca, g.tapR);
    const unsigned gx = (g.w + TW - 1) / TW, gy = (g.h + TH - 1) / TH, tiles = gx * gy * (unsigned)n;
    hipLaunchKernelGGL(k_front, dim3(((tiles + 7u) >> 3) * 8u), dim3(NT), L.bytes, s, b.in, b.mag, b.deg, b.sc, b.pw, b.maxbits, b.ties, b.taps,
                       b.centres, g.W, g.H, g.w, g.h, g.gradThre, L.IWp, (unsigned)L.strip, gx, gy, tiles, clr);
}

}  // namespace lsdhip
