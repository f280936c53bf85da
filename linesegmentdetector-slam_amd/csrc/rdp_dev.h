// rdp_dev.h -- the phases of myrdp::FeatureScan (LSD/myRDP.cpp:9-185 and its callees) that do not depend on how long a scan is.
//
// k_rdp.hip (strides up to 1024, static LDS, two walks by lane 0) and k_rdp_long.hip (1025 .. 4096, dynamic LDS, ordered compactions)
// differ in where the work arrays live, in how the clusters are found and in how the chords are listed.  Everything else is here, once:
// one text, so that the two kernels cannot round apart.  Each phase is called by all 64 lanes of the scan's one wavefront and ends with
// a barrier.  Per scan:
//   1. rdp_metric_gaps: metric coordinates of the readings (lanes) and the gaps between neighbours against the range-dependent
//      threshold (lanes); the clusters are the caller's;
//   2. rdp_split_merge: Ramer-Douglas-Peucker per cluster with an explicit stack: the point of a chord's span farthest from it is found
//      by the 64 lanes (first maximum in scan order, like the reference's strict '>'), the spans to split further go on the stack;
//   3. rdp_pixel_frame: pixel coordinates and their extent (wave min / max); the chords in order are the caller's; rdp_chords: the ones
//      long enough become line records (one lane per line; atand / cosd / sind are the correctly rounded ones of the LSD path), and the
//      pixels of their rasters are listed in the reference's order (line by line; a prefix sum over the lines' pixel counts).
// IEEE corner cases are kept as they are: a vertical chord has an infinite slope, its distances are NaN and nothing is split
// (:245-257); (int) casts of non-finite values follow x86 (cvt_x86).  The reference's read one past its point array (:318-322)
// is of a value it never uses and is not made.
// One host declaration lives here too, because these two files are all that need it: rdp_long_launch, by which launch_rdp (k_rdp.hip)
// reaches the kernels of k_rdp_long.hip.
#pragma once
#include "lsd_internal.h"
#include "devmath.h"

namespace lsdhip {

// k_rdp_long.hip's launch of its two kernels: what launch_rdp (k_rdp.hip) calls for a stride above kRdpShortMaxLen, and nobody else
void rdp_long_launch(const RdpScans& a, const RdpOut& o, hipStream_t s);

// A scan's work arrays in LDS: `len` elements each, stk 2 x len = stk_cap.  The two kernels keep the index type and the push they
// had -- k_rdp `short` and a push without a bound (spans on the stack share end points only, so there are fewer than len of them, and
// its arrays hold 1024), k_rdp_long `unsigned short` and the bound: with them k_rdp's loops compile to the code they were, and the
// latency of one scan, which is what a one-robot tick waits for, is the one it was.
template <class Index, bool kBoundedPush>
struct RdpLds {
    static constexpr bool bounded_push = kBoundedPush;
    using index = Index;
    double *px, *py;                   // metric coordinates, from phase 3 on: pixel coordinates
    Index *cs, *ce;                    // clusters: first and last reading
    Index* stk;                        // the spans still to look at (RDP); before and after that the kernel's own lists
    unsigned char *brk, *split;        // a gap behind the reading; a split point
    int stk_cap;
};

__device__ __forceinline__ double rdp_thre_delta(double val) {                      // getThresholdDeltaDist :347-368
    if (val <= 0.3) return 0.02;
    if (val <= 0.5) return 0.05;
    if (val <= 0.8) return 0.11;
    if (val <= 1) return 0.17;
    if (val <= 2) return 0.6;
    if (val <= 3) return 0.7;
    if (val <= 4) return 0.85;
    if (val <= 5) return 0.9;
    if (val <= 6) return 1;
    return 1.1;
}

// The fleet's form: scan i belongs to sequence i / scans_per_seq, whose map id is map_of[sequence]; the record of that id (uniform per
// workgroup: scalar loads).  An id outside the table: the sequence sits out, its scans get counts 0, nothing else is written, and null
// comes back.
__device__ __forceinline__ const lsd_map_ref* rdp_map_of_scan(const lsd_map_ref* __restrict__ maps, int n_maps, const int32_t* __restrict__ map_of,
                                                              int scans_per_seq, const RdpOut& o) {
    const int id = map_of[blockIdx.x / (unsigned)scans_per_seq];
    if ((unsigned)id < (unsigned)n_maps) return maps + id;
    if (threadIdx.x == 0) { o.n_lines[blockIdx.x] = 0; o.n_pts[blockIdx.x] = 0; }
    return nullptr;
}

// A scan without readings: the six zeros, and true.
__device__ __forceinline__ bool rdp_empty_scan(int len_lp, size_t scan, const RdpOut& o) {
    if (len_lp >= 1) return false;
    if (threadIdx.x == 0) {
        o.n_lines[scan] = 0; o.n_pts[scan] = 0;
        o.lidar_pos[scan * 2] = 0; o.lidar_pos[scan * 2 + 1] = 0; o.im_size[scan * 2] = 0; o.im_size[scan * 2 + 1] = 0;
    }
    return true;
}

// 1. metric coordinates (scanPose = 0, :11) and the gaps; split = 0
template <class Lds>
__device__ __forceinline__ void rdp_metric_gaps(const double* __restrict__ sc /* {range, angle} */, int len_lp, const Lds& w) {
    const int lane = threadIdx.x;
    for (int i = lane; i < len_lp; i += 64) {
        double s, c;
        sincos_g(sc[2 * i + 1] + 0.0, s, c);
        w.px[i] = sc[2 * i] * c + 0.0;                                             // :286-287
        w.py[i] = sc[2 * i] * s + 0.0;
        w.split[i] = 0;
    }
    __syncthreads();
    for (int i = lane; i < len_lp; i += 64) {
        const int nx = i == len_lp - 1 ? 0 : i + 1;                                // :299-306
        const double dX = w.px[i] - w.px[nx], dY = w.py[i] - w.py[nx];
        w.brk[i] = sqrt(dX * dX + dY * dY) > rdp_thre_delta(sc[2 * i]) ? 1 : 0;    // :307-309
    }
    __syncthreads();
}

// 2. SplitMerge :187-217 / SplitMergeAssistant :219-272 over the clusters cs / ce: split[] marks the points found
template <class Lds>
__device__ __forceinline__ void rdp_split_merge(const double* __restrict__ sc, int len_lp, int cells, double thre_line, const Lds& w) {
    using Index = typename Lds::index;
    const int lane = threadIdx.x;
    const double *px = w.px, *py = w.py;
    Index* stk = w.stk;
    for (int cidx = 0; cidx < cells; cidx++) {
        int sp_top = 0;
        if (lane == 0) { stk[0] = w.cs[cidx]; stk[1] = w.ce[cidx]; }
        sp_top = 1;
        __syncthreads();
        while (sp_top > 0) {
            sp_top--;
            const int sp = stk[2 * sp_top], ep = stk[2 * sp_top + 1];
            __syncthreads();
            const int len = ep > sp ? ep - sp + 1 : len_lp + ep - sp + 1;          // :223-239
            if (len <= 2) continue;
            const double k = (py[ep] - py[sp]) / (px[ep] - px[sp]);                // :245-246
            const double d = py[ep] - k * px[ep];
            const double den = sqrt(k * k + 1);
            double best = 0.0;                                                     // dist_max = 0: only a distance > 0 is taken (:257)
            int besto = 0x7fffffff;                                                // its position in the span (first maximum wins)
            for (int i = 1 + lane; i < len - 1; i += 64) {
                int a = sp + i;
                if (a >= len_lp) a -= len_lp;
                const double dist = fabs(k * px[a] - py[a] + d) / den;             // :256
                if (dist > best) { best = dist; besto = i; }                       // (ascending i per lane: the first of equal ones stays)
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int oo = __shfl_xor(besto, off);
                if (ob > best || (ob == best && oo < besto)) { best = ob; besto = oo; }
            }
            int i_max = 0;                                                         // :252 (reading 0 when nothing was farther than 0)
            if (besto != 0x7fffffff) { i_max = sp + besto; if (i_max >= len_lp) i_max -= len_lp; }
            const double r = sc[2 * i_max];
            const double threDist = r > 9 ? r * thre_line : thre_line;             // :259-263
            if (best > threDist && (!Lds::bounded_push || 2 * sp_top + 4 <= w.stk_cap)) {
                if (lane == 0) {
                    stk[2 * sp_top] = (Index)sp; stk[2 * sp_top + 1] = (Index)i_max;
                    stk[2 * sp_top + 2] = (Index)i_max; stk[2 * sp_top + 3] = (Index)ep;
                    w.split[i_max] = 1;
                }
                sp_top += 2;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}

// 3. pixel coordinates (px / py from here on) and the size of the image :16-37; lidar_pos and im_size are written
struct RdpFrame { double minX, minY; int oriXLim, oriYLim; };
template <class Lds>
__device__ __forceinline__ RdpFrame rdp_pixel_frame(int len_lp, double mapResol, double mapOriX, double mapOriY, size_t scan, const RdpOut& o,
                                                    const Lds& w) {
    const int lane = threadIdx.x;
    double minX = INFINITY, minY = INFINITY, maxX = 0, maxY = 0;
    for (int i = lane; i < len_lp; i += 64) {
        const double X = floor((w.px[i] - mapOriX) / mapResol), Y = floor((w.py[i] - mapOriY) / mapResol);
        w.px[i] = X; w.py[i] = Y;
        minX = fmin(minX, X); maxX = fmax(maxX, X); minY = fmin(minY, Y); maxY = fmax(maxY, Y);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        minX = fmin(minX, __shfl_xor(minX, off)); maxX = fmax(maxX, __shfl_xor(maxX, off));
        minY = fmin(minY, __shfl_xor(minY, off)); maxY = fmax(maxY, __shfl_xor(maxY, off));
    }
    const RdpFrame f{minX, minY, cvt_x86(ceil(maxX - minX)), cvt_x86(ceil(maxY - minY))};
    if (lane == 0) {
        o.lidar_pos[scan * 2] = floor((0.0 - mapOriX) / mapResol - minX);          // :35-36
        o.lidar_pos[scan * 2 + 1] = floor((0.0 - mapOriY) / mapResol - minY);
        o.im_size[scan * 2] = f.oriXLim; o.im_size[scan * 2 + 1] = f.oriYLim;
    }
    __syncthreads();
    return f;
}

// The chords of every cluster, in order (:45-71), 64 candidates at a time: candidate ci of first .. n - 1 is a chord where
// chord(ci, a, b) says so, and then from reading a to reading b.  The ones long enough become line records and list the pixels of
// their rasters; then the two counts.
// (the reference puts the first reading in front of the collected split points and the last one behind, :68-69: a flag on one of the
//  two -- flags sit strictly inside a span, so there is none -- would give a chord of length 0 here as there)
template <class Chord, class Lds>
__device__ __forceinline__ void rdp_chords(int first, int n, Chord chord, const RdpFrame& f, double lineDistThre, size_t scan, const RdpOut& o,
                                           const Lds& w) {
    const int lane = threadIdx.x;
    const double minX = f.minX, minY = f.minY;
    const int oriXLim = f.oriXLim, oriYLim = f.oriYLim, pts_cap = o.pts_cap;
    lsd_line* lout = o.lines + scan * (size_t)LSD_RDP_MAX_LINES;                   // line records per scan (the reference's malloc, :39)
    double* pout = o.pts + scan * (size_t)pts_cap * 3;
    int nl = 0, np = 0;                                                            // lines / pixels so far (wave-uniform)
    for (int base = first; base < n; base += 64) {
        const int ci = base + lane;
        bool keep = false;
        double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        int a = 0, b = 0;
        if (ci < n && chord(ci, a, b)) {
            const double ax = w.px[a], ay = w.py[a], bx = w.px[b], by = w.py[b];
            const double ex = ax - bx, ey = ay - by;
            keep = sqrt(ex * ex + ey * ey) >= lineDistThre;                        // :78-79
            x1 = ax - minX; y1 = ay - minY; x2 = bx - minX; y2 = by - minY;        // :81-84
        }
        const unsigned long long km = __ballot(keep);
        const int li = nl + lanes_below(km);
        const double k = (y2 - y1) / (x2 - x1);                                    // :86
        const int xLow = cvt_x86(floor(x1 > x2 ? x2 : x1)), xHigh = cvt_x86(ceil(x1 > x2 ? x1 : x2));   // :94-109
        const int yLow = cvt_x86(floor(y1 > y2 ? y2 : y1)), yHigh = cvt_x86(ceil(y1 > y2 ? y1 : y2));
        const bool along_x = fabs(x2 - x1) > fabs(y2 - y1);                        // :110-115 (integer coordinates: the same as xx_len > yy_len)
        const int cnt = keep ? (along_x ? xHigh - xLow + 1 : yHigh - yLow + 1) : 0;
        // the pixels this line marks (:116-153): count, then place behind the earlier lines' pixels
        int mine = 0;
        for (int m = 0; m < cnt; m++) {
            int xx, yy;
            if (along_x) { xx = m + xLow; yy = cvt_x86(round((xx - x1) * k + y1)); }
            else { yy = m + yLow; xx = cvt_x86(round((yy - y1) / k + x1)); }
            if (!(xx < 0 || xx >= oriXLim || yy < 0 || yy >= oriYLim) && xx != 0 && yy != 0) mine++;   // 0 doubles as "invalid"
        }
        int inc = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (lane >= off) inc += t;
        }
        int wr = np + inc - mine;
        for (int m = 0; m < cnt; m++) {
            int xx, yy;
            if (along_x) { xx = m + xLow; yy = cvt_x86(round((xx - x1) * k + y1)); }
            else { yy = m + yLow; xx = cvt_x86(round((yy - y1) / k + x1)); }
            if (!(xx < 0 || xx >= oriXLim || yy < 0 || yy >= oriYLim) && xx != 0 && yy != 0) {
                if (wr < pts_cap) { pout[3 * (size_t)wr] = xx; pout[3 * (size_t)wr + 1] = yy; pout[3 * (size_t)wr + 2] = 0; }
                wr++;
            }
        }
        if (keep && li < LSD_RDP_MAX_LINES) {
            double ang = atan_g(k) * 180.0 / kPi;                                  // atand, baseFunc.cpp:14-16
            int orient = 1;
            if (ang < 0) { ang += 180; orient = -1; }                              // :89-92
            lsd_line L;
            L.k = k;
            L.b = (y1 + y2) / 2.0 - k * (x1 + x2) / 2.0;                           // :164
            sincos_g(ang / 180.0 * kPi, L.dy, L.dx);                               // sind / cosd
            L.x1 = x1; L.y1 = y1; L.x2 = x2; L.y2 = y2;
            const double ey = y2 - y1, ex = x2 - x1;
            L.len = sqrt(ey * ey + ex * ex);                                       // :171
            L.orient = orient;
            lout[li] = L;
            reinterpret_cast<uint32_t*>(&lout[li])[19] = 0u;                       // the tail padding: defined bytes
        }
        nl += __builtin_popcountll(km);
        np += __shfl(inc, 63);
    }
    if (lane == 0) { o.n_lines[scan] = nl; o.n_pts[scan] = np; }
}

}  // namespace lsdhip
