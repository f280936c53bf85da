// k_rdp_long.hip -- myrdp::FeatureScan for scans of 1025 .. 4096 readings (gfx950): one wavefront per scan, dynamic LDS.
//
// The same function as k_rdp.hip (LSD/myRDP.cpp:9-185 with RegionSegmentation, SplitMerge, SplitMergeAssistant and
// getThresholdDeltaDist), the same outputs at the same strides, the same bits; launch_rdp / launch_rdp_maps send a launch here when its
// stride is above k_rdp's 1024.  What differs:
//   - the work arrays are dynamic LDS sized from the launch's stride (k_rdp_lds.h: 26 bytes per reading), indices are 16 bits wide;
//   - no lane walks over all readings.  k_rdp's two walks by lane 0 -- RegionSegmentation's cluster walk and the listing of the chords
//     -- are ordered compactions here (ballot + the kept lanes below, over chunks of 64, the idiom of k_ingest):
//       clusters  the readings behind which the gap is over the threshold are listed in order (B); run j is [B[j-1] + 1, B[j]] (the first
//                 from 0); the reference writes a run at cs[cellNumber] and moves on only if abs(i - startNum) >= region_point_limit,
//                 so the clusters are the runs that pass that test, in order -- a second compaction over B; where the last reading
//                 has no gap behind it, cs[0] = B[last] + 1 (0 without a gap anywhere): the last run joins cluster 0, whichever
//                 run that is;
//       chords    the clusters are disjoint and ascending, except that a joined cluster 0 starts behind every other one and runs
//                 through the end of the scan: in the order (reading - cs[0]) mod len, clusters and the readings inside them both
//                 ascend.  Each reading lists itself once as its cluster's first reading, once as a split point, once as its
//                 cluster's last reading (P, a compaction in that order); the chords are the neighbours (P[t-1], P[t]) where P[t]
//                 does not begin a cluster.
//     The RDP stack loop and the per-line raster loops are k_rdp's.
// One wavefront, not four: the batch is the parallelism (one scan per workgroup, hundreds of scans per launch), the farthest-point
// search keeps k_rdp's shuffle reduction with its first-maximum rule, and the barriers stay wave-local.
// Kept as they are: everything k_rdp.hip's head lists (vertical chords with NaN distances, cvt_x86, 0 doubling as "invalid" in the
// raster, len_lp < 1 writing the six zeros, the first maximum under the strict '>').  Line records stay at 360 per scan: a scan with
// more reports the full count and stores the first 360.
// Domain: region_point_limit >= 1, the reference's.  Below 1 a cluster of ONE reading can exist, whose span the reference takes for
// the whole scan plus one (its wrap-around formula at ep == sp); that is not restated here -- such a cluster gives one chord of
// length 0 -- and every index stays inside its array.
#include "lsd_internal.h"
#include "devmath.h"
#include "k_rdp_lds.h"

namespace lsdhip {

constexpr int kRdpLongMaxLines = 360;               // line records per scan (k_rdp's kRdpMaxLines)
constexpr unsigned kFirstOfCluster = 0x8000u;       // flag on an entry of P

extern __shared__ double rdp_long_lds_base[];

__device__ __forceinline__ double rdp_long_thre_delta(double val) {                 // getThresholdDeltaDist :347-368
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

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// One scan (blockIdx.x) with the map's resolution and origin given: the body of both kernels below.
__device__ __forceinline__ void rdp_long_scan(const double* __restrict__ scans /* n x stride x {range, angle} */, const int* __restrict__ lens,
                                              int stride, double mapResol, double mapOriX, double mapOriY, int region_point_limit,
                                              double thre_line, double line_dist_thre_m, lsd_line* __restrict__ lines_out,
                                              int* __restrict__ n_lines, double* __restrict__ pts_out, int pts_cap, int* __restrict__ n_pts,
                                              double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    // the launch's dynamic LDS, rdp_long_lds(stride) bytes: every array holds `stride` elements (stk: 2 x stride)
    double* px = rdp_long_lds_base;
    double* py = px + stride;
    unsigned short* cs = reinterpret_cast<unsigned short*>(py + stride);           // clusters: first and last reading
    unsigned short* ce = cs + stride;
    unsigned short* stk = ce + stride;                 // in turn: the breaks B, the spans still to look at (RDP), the chord points P
    unsigned char* brk = reinterpret_cast<unsigned char*>(stk + 2 * stride);       // a gap behind the reading; later: first / last of a cluster
    unsigned char* split = brk + stride;
    const int stk_cap = 2 * stride;
    const size_t scan = blockIdx.x;
    const int lane = threadIdx.x;
    const int len_lp = min(lens[scan], stride);
    const double* sc = scans + scan * (size_t)stride * 2;
    lsd_line* lout = lines_out + scan * (size_t)kRdpLongMaxLines;
    double* pout = pts_out + scan * (size_t)pts_cap * 3;
    if (len_lp < 1) {
        if (lane == 0) { n_lines[scan] = 0; n_pts[scan] = 0; lidar_pos[scan * 2] = 0; lidar_pos[scan * 2 + 1] = 0; im_size[scan * 2] = 0; im_size[scan * 2 + 1] = 0; }
        return;
    }
    // 1. metric coordinates (scanPose = 0, :11) and the gaps
    for (int i = lane; i < len_lp; i += 64) {
        double s, c;
        sincos_g(sc[2 * i + 1] + 0.0, s, c);
        px[i] = sc[2 * i] * c + 0.0;                                               // :286-287
        py[i] = sc[2 * i] * s + 0.0;
        split[i] = 0;
    }
    __syncthreads();
    for (int i = lane; i < len_lp; i += 64) {
        const int nx = i == len_lp - 1 ? 0 : i + 1;                                // :299-306
        const double dX = px[i] - px[nx], dY = py[i] - py[nx];
        brk[i] = sqrt(dX * dX + dY * dY) > rdp_long_thre_delta(sc[2 * i]) ? 1 : 0; // :307-309
    }
    __syncthreads();
    // RegionSegmentation's walk :297-330 as two compactions.  B: the readings with a gap behind them, in order
    int nb = 0;
    for (int c0 = 0; c0 < len_lp; c0 += 64) {
        const int i = c0 + lane;
        const bool b = i < len_lp && brk[i];
        const unsigned long long m = __ballot(b);
        if (b) stk[nb + lanes_below(m)] = (unsigned short)i;                       // nb + below <= i < stride
        nb += __builtin_popcountll(m);
    }
    const bool joins = !brk[len_lp - 1];                                           // the last run joins cluster 0 (:361-365)
    __syncthreads();
    // the runs [B[j-1] + 1, B[j]] that are long enough, in order: the clusters
    int cells = 0;
    for (int c0 = 0; c0 < nb; c0 += 64) {
        const int j = c0 + lane;
        int startNum = 0, i = 0;
        bool keep = false;
        if (j < nb) {
            i = stk[j];
            startNum = j ? stk[j - 1] + 1 : 0;
            keep = abs(i - startNum) >= region_point_limit;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) { const int at = cells + lanes_below(m); cs[at] = (unsigned short)startNum; ce[at] = (unsigned short)i; }   // at <= j < stride
        cells += __builtin_popcountll(m);
    }
    const int lastStart = nb ? stk[nb - 1] + 1 : 0;                                // startNum when the walk ends
    __syncthreads();
    if (joins && cells > 0 && lane == 0) cs[0] = (unsigned short)lastStart;        // (lastStart <= len_lp - 1: the last reading is no break)
    __syncthreads();
    // 2. SplitMerge :187-217 / SplitMergeAssistant :219-272 (k_rdp's loop)
    for (int cidx = 0; cidx < cells; cidx++) {
        int sp_top = 0;
        if (lane == 0) { stk[0] = cs[cidx]; stk[1] = ce[cidx]; }
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
            if (best > threDist && 2 * sp_top + 4 <= stk_cap) {                    // (spans on the stack share end points only: < len_lp of them)
                if (lane == 0) {
                    stk[2 * sp_top] = (unsigned short)sp; stk[2 * sp_top + 1] = (unsigned short)i_max;
                    stk[2 * sp_top + 2] = (unsigned short)i_max; stk[2 * sp_top + 3] = (unsigned short)ep;
                    split[i_max] = 1;
                }
                sp_top += 2;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // 3. pixel coordinates and the size of the image :16-37
    double minX = INFINITY, minY = INFINITY, maxX = 0, maxY = 0;
    for (int i = lane; i < len_lp; i += 64) {
        const double X = floor((px[i] - mapOriX) / mapResol), Y = floor((py[i] - mapOriY) / mapResol);
        px[i] = X; py[i] = Y;
        minX = fmin(minX, X); maxX = fmax(maxX, X); minY = fmin(minY, Y); maxY = fmax(maxY, Y);
        brk[i] = 0;                                                                // from here: 1 = first reading of a cluster, 2 = last
    }
    for (int off = 32; off >= 1; off >>= 1) {
        minX = fmin(minX, __shfl_xor(minX, off)); maxX = fmax(maxX, __shfl_xor(maxX, off));
        minY = fmin(minY, __shfl_xor(minY, off)); maxY = fmax(maxY, __shfl_xor(maxY, off));
    }
    const int oriXLim = cvt_x86(ceil(maxX - minX)), oriYLim = cvt_x86(ceil(maxY - minY));
    if (lane == 0) {
        lidar_pos[scan * 2] = floor((0.0 - mapOriX) / mapResol - minX);            // :35-36
        lidar_pos[scan * 2 + 1] = floor((0.0 - mapOriY) / mapResol - minY);
        im_size[scan * 2] = oriXLim; im_size[scan * 2 + 1] = oriYLim;
    }
    __syncthreads();
    for (int c = lane; c < cells; c += 64) brk[cs[c]] = 1;                         // (the clusters are disjoint: one writer per reading)
    __syncthreads();
    for (int c = lane; c < cells; c += 64) brk[ce[c]] |= 2;
    __syncthreads();
    // the chord points of every cluster, in order (:45-71): its first reading, its split points, its last reading -> P
    const int rot = joins && cells > 0 ? cs[0] : 0;
    int n_p = 0;
    for (int c0 = 0; c0 < len_lp; c0 += 64) {
        const int r = c0 + lane;
        int v = 0;
        bool first = false, mid = false, last = false;
        if (r < len_lp) {
            v = r + rot;
            if (v >= len_lp) v -= len_lp;
            first = brk[v] & 1; mid = split[v]; last = brk[v] & 2;
        }
        const unsigned long long mf = __ballot(first), mm = __ballot(mid), ml = __ballot(last);
        int at = n_p + lanes_below(mf) + lanes_below(mm) + lanes_below(ml);
        if (first) { if (at < stk_cap) stk[at] = (unsigned short)(v | kFirstOfCluster); at++; }
        if (mid) { if (at < stk_cap) stk[at] = (unsigned short)v; at++; }
        if (last) { if (at < stk_cap) stk[at] = (unsigned short)v; }
        n_p += __builtin_popcountll(mf) + __builtin_popcountll(mm) + __builtin_popcountll(ml);
    }
    n_p = min(n_p, stk_cap);                                                       // (in the domain n_p <= len_lp: a reading is one of the three)
    __syncthreads();
    // (the reference puts the first reading in front of the collected split points and the last one behind, :68-69)
    const double lineDistThre = line_dist_thre_m / mapResol;
    int nl = 0, np = 0;                                                            // lines / pixels so far (wave-uniform)
    for (int base = 1; base < n_p; base += 64) {
        const int ci = base + lane;
        bool keep = false;
        double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (ci < n_p && !(stk[ci] & kFirstOfCluster)) {                            // the chord (P[ci - 1], P[ci])
            const int a = stk[ci - 1] & (kFirstOfCluster - 1u), b = stk[ci];
            const double ax = px[a], ay = py[a], bx = px[b], by = py[b];
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
        if (keep && li < kRdpLongMaxLines) {
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
    if (lane == 0) { n_lines[scan] = nl; n_pts[scan] = np; }
}

__global__ __launch_bounds__(64) void k_rdp_long(const double* __restrict__ scans, const int* __restrict__ lens, int stride, double mapResol,
                                                 double mapOriX, double mapOriY, int region_point_limit, double thre_line,
                                                 double line_dist_thre_m, lsd_line* __restrict__ lines_out, int* __restrict__ n_lines,
                                                 double* __restrict__ pts_out, int pts_cap, int* __restrict__ n_pts,
                                                 double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    rdp_long_scan(scans, lens, stride, mapResol, mapOriX, mapOriY, region_point_limit, thre_line, line_dist_thre_m, lines_out, n_lines,
                  pts_out, pts_cap, n_pts, lidar_pos, im_size);
}

// The fleet's form (k_rdp_maps): an id outside the table -> the sequence sits out, its scans get counts 0 and nothing else is written.
__global__ __launch_bounds__(64) void k_rdp_maps_long(const double* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                      const lsd_map_ref* __restrict__ maps, int n_maps, const int32_t* __restrict__ map_of,
                                                      int scans_per_seq, int region_point_limit, double thre_line, double line_dist_thre_m,
                                                      lsd_line* __restrict__ lines_out, int* __restrict__ n_lines,
                                                      double* __restrict__ pts_out, int pts_cap, int* __restrict__ n_pts,
                                                      double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    const int id = map_of[blockIdx.x / (unsigned)scans_per_seq];
    if ((unsigned)id >= (unsigned)n_maps) {
        if (threadIdx.x == 0) { n_lines[blockIdx.x] = 0; n_pts[blockIdx.x] = 0; }
        return;
    }
    const lsd_map_ref* __restrict__ m = maps + id;
    rdp_long_scan(scans, lens, stride, m->mapResol, m->mapOriX, m->mapOriY, region_point_limit, thre_line, line_dist_thre_m, lines_out,
                  n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size);
}

// Once per context, before its first long launch: LDS above 64 KiB needs the kernels' dynamic-LDS limit raised (lsd_set_scan_capacity
// has checked the size against the device's limit).  An error here leaves nothing queued.
hipError_t prepare_rdp_long(size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rdp_long), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_rdp_maps_long), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

void launch_rdp_long(const double* scans, const int* lens, int n, int stride, double mapResol, double mapOriX, double mapOriY,
                     int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line* lines_out, int* n_lines, double* pts_out,
                     int pts_cap, int* n_pts, double* lidar_pos, int* im_size, hipStream_t s) {
    hipLaunchKernelGGL(k_rdp_long, dim3(n), dim3(64), rdp_long_lds(stride), s, scans, lens, stride, mapResol, mapOriX, mapOriY,
                       region_point_limit, thre_line, line_dist_thre_m, lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size);
}
void launch_rdp_maps_long(const double* scans, const int* lens, int n, int stride, const lsd_map_ref* maps, int n_maps, const int32_t* map_of,
                          int scans_per_seq, int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line* lines_out,
                          int* n_lines, double* pts_out, int pts_cap, int* n_pts, double* lidar_pos, int* im_size, hipStream_t s) {
    hipLaunchKernelGGL(k_rdp_maps_long, dim3(n), dim3(64), rdp_long_lds(stride), s, scans, lens, stride, maps, n_maps, map_of, scans_per_seq,
                       region_point_limit, thre_line, line_dist_thre_m, lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size);
}

}  // namespace lsdhip
