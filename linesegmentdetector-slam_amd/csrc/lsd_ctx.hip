// lsd_ctx.hip -- host side of liblsdhip.so: context, HBM workspace, host-computed tables, launch
// sequencing and the detector's, the map cache's and the map update's part of the C ABI declared in
// include/lsd_hip.h (localisation: lsd_loc.hip; the grid stack: lsd_grid.hip; the pose graph: lsd_pg.hip).
//
// Everything numerical on the hot path runs in the HIP kernels (k_*.hip).  The host computes only
// what the reference also computes once per call on scalars: the Gaussian taps (myLSD.cpp:398-417),
// the thresholds (myLSD.cpp:148-149, :207-209) and two small lookup tables (log-gamma of integers,
// logs of p = aliPro/2^k) that the kernels index instead of evaluating libm on the device.
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "lsd_ctx.h"
#include "k1_lds.h"
#include "k_rdp_lds.h"

using namespace lsdhip;

constexpr size_t kPinBytes = 32u << 20;   // two pinned staging buffers of this size per context

// ---------------------------------------------------------------------------------------------
// host-computed scalars and tables
// ---------------------------------------------------------------------------------------------
static int tap_radius(double sca, double sig) {                     // myLSD.cpp:390-393
    const int prec = 3;
    if (sca < 1) sig = sig / sca;
    return cvt_x86(ceil(sig * sqrt(2 * prec * log(10))));
}

static void gauss_taps(double sca, double sig, int h, std::vector<double>& t) {   // myLSD.cpp:398-417
    if (sca < 1) sig = sig / sca;
    const int hSize = 1 + 2 * h;
    t.assign((size_t)3 * hSize, 0.0);
    double s1 = 0, s2 = 0, s3 = 0;
    for (int k = 0; k < hSize; k++) {
        const double a = (k - h) / sig, b = (k - h - 1.0 / 3) / sig, c = (k - h + 1.0 / 3) / sig;
        t[0 * hSize + k] = exp(-0.5 * (a * a));
        t[1 * hSize + k] = exp(-0.5 * (b * b));
        t[2 * hSize + k] = exp(-0.5 * (c * c));
        s1 += t[0 * hSize + k]; s2 += t[1 * hSize + k]; s3 += t[2 * hSize + k];
    }
    for (int k = 0; k < hSize; k++) {
        t[0 * hSize + k] /= s1; t[1 * hSize + k] /= s2; t[2 * hSize + k] /= s3;
    }
}

static double log_gamma_host(int x) {                               // LogGammaCalculator, myLSD.cpp:882-924
    if (x > 15)
        return 0.918938533204673 + (x - 0.5) * log(x) - x + 0.5 * x * log(x * sinh(1.0 / x) + 1.0 / (810 * pow(x, 6)));
    static const double q[7] = {75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705,
                                1168.92649479, 83.8676043424, 2.50662827511};
    double a = (x + 0.5) * log(x + 5.5) - (x + 5.5), b = 0;
    for (int i = 0; i < 7; i++) { a -= log(x + i); b += q[i] * pow(x, i); }
    return a + log(b);
}

// LogGammaCalculator(0 .. count - 1) from the host libm, computed once per process (a 2048 x 2048 map needs 377 k entries: ~40 ms)
static std::mutex g_lg_mu;                                          // held while the table is grown and while a context copies out of it
static const double* log_gamma_table(int count) {
    static std::vector<double> tab;
    if ((int)tab.size() < count) {
        const int from = (int)tab.size();
        tab.resize(count);
        for (int i = from; i < count; i++) tab[i] = i >= 1 ? log_gamma_host(i) : 0.0;
    }
    return tab.data();
}

// c: the context whose device has to launch K1 on this geometry (its LDS limit, and lsd_last_error for that refusal)
static int make_geom(lsd_ctx* c, const lsd_params* p, int cols, int rows, Geom* g) {
    if (!p || cols <= 0 || rows <= 0) return LSD_ERR_INVALID;
    if (!(p->sca > 0) || !(p->sig > 0) || !(p->angThre > 0) || p->pseBin < 1) return LSD_ERR_INVALID;
    if (p->pseBin > 1024) return LSD_ERR_UNSUPPORTED;
    if (cols > 65535 || rows > 65535) return LSD_ERR_UNSUPPORTED;
    g->W = cols; g->H = rows;
    g->w = cvt_x86(floor(cols * p->sca));                           // myLSD.cpp:132
    g->h = cvt_x86(floor(rows * p->sca));                           // :133
    if (g->w < 2 || g->h < 2) return LSD_ERR_INVALID;
    // the region stage packs scaled coordinates as (y<<16 | x) and keeps bounding boxes (+-1 margin) in 16-bit signed fields
    if (g->w > 32766 || g->h > 32766) return LSD_ERR_UNSUPPORTED;
    if ((long long)g->w * g->h > (1ll << 30)) return LSD_ERR_UNSUPPORTED;
    g->npx = g->w * g->h;
    g->gp = (g->w + 15) & ~15;
    g->sca = p->sca;
    g->tapR = tap_radius(p->sca, p->sig);
    if (g->tapR < 0 || g->tapR > kMaxTapRadius) return LSD_ERR_UNSUPPORTED;
    // K1 stages a tile's whole source window in LDS (k1_lds.h): ~(23 / sca + 2 tapR) rows of (31 / sca + 2 tapR) bytes and 32 doubles.
    // A window beyond what a workgroup of this device may have could not be launched: refused here, before anything is enqueued.
    const size_t k1_bytes = k1_lds(p->sca, g->tapR).bytes;
    if (k1_bytes > c->max_lds) {
        char msg[200];
        snprintf(msg, sizeof msg, "sca = %g, sig = %g: the Gaussian's window needs %zu bytes of LDS per workgroup, the device has %zu",
                 p->sca, p->sig, k1_bytes, c->max_lds);
        c->err = msg;
        return LSD_ERR_UNSUPPORTED;
    }
    g->pseBin = p->pseBin;
    g->degThre = p->angThre / 180.0 * kPi;                          // :148
    g->gradThre = 2.0 / sin(g->degThre);                            // :149
    g->logNT = 5 * (log10(g->h) + log10(g->w)) / 2.0;               // :207
    g->regThre = -g->logNT / log10(p->angThre / 180.0);             // :208
    g->aliPro = p->angThre / 180.0;                                 // :209
    g->denThre = p->denThre;
    return LSD_OK;
}

static int ensure_tables(lsd_ctx* c, const lsd_params* p, const Geom& g, hipStream_t s) {
    // log-gamma of every pixel count a rectangle of this geometry can have (all + 1 <= w*h + 1, myLSD.cpp:1030): host libm values, as
    // the reference computes them; the device only looks them up
    const int lg_need = (int)std::min<long long>(std::max<long long>((long long)g.npx + 2, kLgTable), kLgTableMax);
    if ((int)c->d_lgamma.capacity() < lg_need) {
        HIPCHK(c, hipStreamSynchronize(s));
        if (c->done_valid) HIPCHK(c, hipEventSynchronize(c->ev_done));
        std::lock_guard<std::mutex> lk(g_lg_mu);
        const double* tab = log_gamma_table(lg_need);
        HIPCHK(c, c->d_lgamma.resize(lg_need));
        const hipError_t e = hipMemcpy(c->d_lgamma.get(), tab, sizeof(double) * lg_need, hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)c->d_lgamma.resize(0);           // (its capacity says how much of the table is on the device)
        HIPCHK(c, e);
    }
    if (c->tab_valid && memcmp(&c->tab_params, p, sizeof(lsd_params)) == 0) return LSD_OK;
    if (!c->d_ptab.get()) {
        HIPCHK(c, c->d_ptab.resize(kPTable * 3));
        HIPCHK(c, c->d_taps.resize(3 * (2 * kMaxTapRadius + 1)));
        HIPCHK(c, c->d_centres.resize(kCentreCount));
    }
    std::vector<double> taps;
    gauss_taps(p->sca, p->sig, g.tapR, taps);
    std::vector<int> centres(kCentreCount);                         // myLSD.cpp:428 / :460, the host's own division and rounding
    for (int x = 0; x < kCentreCount; x++) centres[x] = cvt_x86(floor(x / p->sca + 0.5));
    double pt[kPTable * 3];
    double pr = g.aliPro;
    for (int k = 0; k < kPTable; k++) {
        pt[k * 3 + 0] = log(pr); pt[k * 3 + 1] = log10(pr); pt[k * 3 + 2] = log(1 - pr);   // myLSD.cpp:1024,:1033
        pr /= 2.0;                                                                          // :1085,:1149
    }
    HIPCHK(c, hipStreamSynchronize(s));
    // kernels of an earlier enqueue (on whatever stream, which may be gone by now) may still read the tables: wait for the event
    // that enqueue recorded, never for its stream
    if (c->done_valid) HIPCHK(c, hipEventSynchronize(c->ev_done));
    HIPCHK(c, hipMemcpy(c->d_taps.get(), taps.data(), sizeof(double) * taps.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_ptab.get(), pt, sizeof(pt), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_centres.get(), centres.data(), sizeof(int) * kCentreCount, hipMemcpyHostToDevice));
    c->tab_params = *p;
    c->tab_valid = true;
    c->tapR = g.tapR;
    return LSD_OK;
}

// wavefronts per image of the region-stage build a batch of n images runs on (see launch below)
static int waves_for(const lsd_ctx* c, int n) {
    // 8 wavefronts per image (one image per CU) finish an image ~1.5x sooner; 4 (two images per CU) have the higher throughput.
    // While the batch is only a few images per CU its time is that of its heaviest images: 8.  Long batches: 4.
    // (the per-wave workspace -- stamps / spill / gcopy, 12 B per scaled pixel and wave, + result slots -- doubles with 8 waves:
    //  the whole workspace is 56 MB per 2048^2 map on 8 waves and 40 MB on 4 (tools/workspace_size.py: 28.6 / 20.3 GB for the bench
    //  batch of 512); if the 8-wave workspace cannot be allocated the context falls back to 4)
    if (c->region_waves_mode == 8 || (c->region_waves_mode == 0 && !c->prefer4 && n <= 4 * c->num_cus)) return 8;
    return 4;
}

// Workgroups that own no image and help from the start (k_region.hip): as many as the images leave workgroup slots of the device
// free -- one 8-wave workgroup per CU, three 4-wave ones -- and the images' helper wavefronts (tun_help each) can use.
constexpr int kPoolHelpMax = 64;        // helper wavefronts per image the pool is sized for at most (workspace: a wave slot each)
static int pool_for(const lsd_ctx* c, int n, int help) {
    if (help < 0) help = 24;
    if (help > kPoolHelpMax) help = kPoolHelpMax;
    // Measured (tools/single_step_probe.py): the heaviest bench image alone 77.5 -> 30 ms, typical single images unchanged (they never
    // ask: tun_gate); a 64-image shard 49 -> 55 ms and the 512-image batch on 4 waves 87 -> 115 ms -- helpers that are there from the
    // start serve many images that merely look busy, and every remote evaluation costs its owner an export, a poll and a validation
    // out of HBM.  So the pool exists for calls with a handful of images (the reference's usage: one map per call); batches get their
    // helpers from the workgroups that finish first, as before.
    if (help <= 0 || c->trace || n > c->pool_max_images) return 0;
    const int nw = waves_for(c, n);
    const long long free_slots = (long long)(nw == 8 ? 1 : 3) * c->num_cus - n;
    const long long want = ((long long)n * help + nw - 1) / nw;
    const long long p = free_slots < want ? free_slots : want;
    return p > 0 ? (int)p : 0;
}
static int pool_for(const lsd_ctx* c, int n) { return pool_for(c, n, c->tun_help); }
// ... and what the workspace is sized for: the pool of the default help setting even while help is switched off, so that switching
// it on later (lsd_set_region_help) never makes the never-allocating entry point allocate
static int pool_reserve_for(const lsd_ctx* c, int n) {
    const int now = c->tun_help < 0 ? 24 : c->tun_help;
    return pool_for(c, n, now > 24 ? now : 24);
}

// Does a call with this geometry take the fused front end (k_front.hip)?  The reference's 17 taps, a pipeline that runs at least as far
// as the gradient pass, no seed trace, and its LDS fits; everything else runs K1 and K2 as two kernels.
static bool use_front(const lsd_ctx* c, const Geom& g) {
    return c->fused_front && !c->trace && (c->stop_after == 0 || c->stop_after >= LSD_STAGE_GRAD) && front_fits(g, c->max_lds);
}
// ... and the Gaussian elements per image its workspace needs: none on the fused path (1.55 GB per context at 512 maps of 2048^2)
static size_t gauss_elems(const lsd_ctx* c, const Geom& g) { return use_front(c, g) ? 0 : (size_t)g.gp * g.h; }

// Words per wave of the member-mask array (4 per 8x8 tile) for any image of up to npx scaled pixels: tiles <= npx / 64 + (w + h) / 8 + 1,
// and w, h <= 32766 (make_geom).
static size_t tm_words(size_t npx) { return npx / 16 + 4 * 8200; }

static int ensure_workspace_impl(lsd_ctx* c, size_t n, size_t npx, size_t gpx, int max_lines, bool trace) {
    Workspace& w = c->ws;
    const size_t need_ws = (n + (size_t)pool_reserve_for(c, (int)n)) * (size_t)waves_for(c, (int)n);   // per-wave arrays: wave slots of the images and of the helper pool
    const bool grow_main = n > w.cap_n || npx > w.cap_npx || gpx > w.cap_gpx || need_ws > w.cap_ws;
    if (grow_main) {
        const size_t nn = n > w.cap_n ? n : w.cap_n, pp = npx > w.cap_npx ? npx : w.cap_npx;
        const size_t gg = gpx > w.cap_gpx ? gpx : w.cap_gpx;
        const size_t ws = need_ws > w.cap_ws ? need_ws : w.cap_ws;
        HIPCHK(c, hipDeviceSynchronize());
        const size_t tot = nn * pp;
        HIPCHK(c, w.gauss.resize(nn * gg)); HIPCHK(c, w.mag.resize(tot)); HIPCHK(c, w.deg.resize(tot));
        HIPCHK(c, w.sc.resize(tot));
        HIPCHK(c, w.pw.resize(tot)); HIPCHK(c, w.epochmap.resize(tot)); HIPCHK(c, w.ord.resize(tot));
        HIPCHK(c, w.spill.resize(ws * pp)); HIPCHK(c, w.gcopy.resize(ws * pp)); HIPCHK(c, w.wmeta.resize(ws * (size_t)c->mcap));
        HIPCHK(c, w.stamps.resize(ws * tm_words(pp))); HIPCHK(c, w.seedidx.resize(tot)); HIPCHK(c, w.seedpos.resize(tot)); HIPCHK(c, w.tepoch.resize(nn * (pp / 16 + 4096)));
        HIPCHK(c, hipMemset(w.stamps.get(), 0, ws * tm_words(pp) * sizeof(uint32_t)));
        HIPCHK(c, hipMemset(w.epochmap.get(), 0, tot * sizeof(uint32_t)));
        w.run_id = 0;
        const size_t gs = ws * (size_t)region_slots();                          // result slots: NS per wave slot
        HIPCHK(c, w.slist.resize(gs * (size_t)c->gcap));
        HIPCHK(c, w.pend.resize(gs * 24));
        HIPCHK(c, w.order.resize(nn));
        HIPCHK(c, w.sets.resize(nn * 256));
        HIPCHK(c, w.xq.resize(nn * (size_t)(kXStride + 1) + kXHdr));
        HIPCHK(c, w.maxbits.resize(nn + (nn + 1) / 2)); HIPCHK(c, w.nb.resize(nn)); HIPCHK(c, w.nseed.resize(nn));   // (maxbits: [0, nn) the maxima, then nn int32: the gradient pass's near-tie counts -- one memset clears both)
        HIPCHK(c, w.stats.resize(nn * kStatWords)); HIPCHK(c, w.rnum.resize(nn * (size_t)region_ring() * 2));
        HIPCHK(c, w.seeds.resize(0));
        if (nn != w.cap_n) { w.cap_max_lines = 0; }
        w.cap_n = nn; w.cap_npx = pp; w.cap_gpx = gg; w.cap_ws = ws;
    }
    if (max_lines > w.cap_max_lines) {
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, w.recs.resize(w.cap_n * (size_t)max_lines * 12));
        HIPCHK(c, w.recs_scaled.resize(w.cap_n * (size_t)max_lines * 4));
        w.cap_max_lines = max_lines;
    }
    if (trace && !w.seeds.get()) {
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, w.seeds.resize(w.cap_n * w.cap_npx));
    }
    return LSD_OK;
}

// A failed (re)allocation leaves some arrays freed and others at their old size: forget the whole workspace, so that the next
// call starts from nothing instead of trusting stale capacities.
static int ensure_workspace(lsd_ctx* c, size_t n, size_t npx, size_t gpx, int max_lines, bool trace) {
    int st = ensure_workspace_impl(c, n, npx, gpx, max_lines, trace);
    if (st != LSD_OK) {
        (void)hipGetLastError();                                      // the failed allocation is sticky otherwise
        c->ws = Workspace{};
        if (st == LSD_ERR_NOMEM && c->region_waves_mode == 0 && !c->prefer4 && waves_for(c, (int)n) == 8) {
            // the 8-wave variant's workspace does not fit: once more with 4 wavefronts per image (half the per-wave arrays)
            c->prefer4 = true;
            return ensure_workspace(c, n, npx, gpx, max_lines, trace);
        }
    }
    return st;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// The schedule settings of the region stage by name (see lsd_create / lsd_debug_set_tuning)
struct Tuning { const char* name; int lo, hi; int lsd_ctx::*field; bool shipped; };
static const Tuning kTunings[] = {
    {"HELP", -1, 4096, &lsd_ctx::tun_help, true},          // helper wavefronts per image (as lsd_set_region_help)
    {"POOL", 0, 16, &lsd_ctx::pool_max_images, true},      // calls with at most this many images get helper-only workgroups
    {"SOFT", 0, 1 << 20, &lsd_ctx::tun_soft, false},       // look-ahead of the seed hand-out, shallow / deep end (seeds; 0: default)
    {"CLAIM", 0, 1 << 20, &lsd_ctx::tun_claim, false},
    {"FEED", 1, 8, &lsd_ctx::tun_feed, false},             // idle lane groups per refill
    {"BIG", 0, 16, &lsd_ctx::tun_big, false},              // results a wave may have waiting for the cursor (0: default)
    {"EARLY", 0, 4096, &lsd_ctx::tun_early, false},        // helpers before every workgroup has its CU (measured: a loss)
    {"WB", 0, 100, &lsd_ctx::tun_wb, false},               // idle share (%) below which an image asks for help
    {"GATE", 0, 1 << 22, &lsd_ctx::tun_gate, false},       // ... once it has been running for this long (x 1024 clocks)
    {"SHARE", 0, 100, &lsd_ctx::tun_share, false},
    {"UP", 0, 1 << 16, &lsd_ctx::tun_up, false},           // steps of the adaptive look-ahead
    {"DOWN", 0, 1 << 16, &lsd_ctx::tun_down, false},
    {"REQUEUE", 0, 1, &lsd_ctx::tun_requeue, false},       // 0: invalidated results are found at the cursor only
    {"XPOLL", 100, 1 << 30, &lsd_ctx::tun_xpoll, false},   // clocks between two looks of a wave at the help protocol
    {"LINGER", 1, 1 << 30, &lsd_ctx::tun_linger, false},   // looks (~27 us each) a helper takes for an image that asks before it gives its CU back
    {"GROUPS", -1, 1 << 20, &lsd_ctx::tun_groups, false},  // 8-wave region stage as persistent workgroups: -1 (default) as many as CUs when the batch has more images, 0 never, n that many
    {"STOP", 0, 1 << 30, &lsd_ctx::tun_stop, false},       // developer build of the kernel: the seed loop ends after this many seeds (probe experiment)
    {"FA_LDS", 0, kFaLdsMax, &lsd_ctx::fa_lds_bound, false},   // FeatureAssociation: kept candidates up to which the sort runs in LDS (tests reach the global path)
};

extern "C" {

int lsd_abi_version(void) { return LSD_ABI_VERSION; }

const char* lsd_strerror(int st) {
    switch (st) {
        case LSD_OK: return "ok";
        case LSD_ERR_INVALID: return "invalid argument";
        case LSD_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
        case LSD_ERR_HIP: return "HIP runtime error";
        case LSD_ERR_UNSUPPORTED: return "parameter outside the implemented range";
        case LSD_ERR_CAPACITY: return "line capacity exceeded";
        case LSD_ERR_NOMEM: return "out of memory (host or device)";
        case LSD_ERR_INTERNAL: return "the region stage gave an image up (its watchdog; see lsd_last_error)";
        default: return "unknown status";
    }
}

void lsd_default_params(lsd_params* p) {                            // LSD/baseFunc.h:64-68
    if (!p) return;
    p->sca = 0.3; p->sig = 0.6; p->angThre = 22.5; p->denThre = 0.7; p->pseBin = 1024;
}

void lsd_scaled_size(int cols, int rows, double sca, int* w, int* h) {
    if (w) *w = cvt_x86(floor(cols * sca));
    if (h) *h = cvt_x86(floor(rows * sca));
}

int lsd_create(lsd_ctx** out, int device) {
    if (!out) return LSD_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return LSD_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return LSD_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return LSD_ERR_NO_DEVICE;
    lsd_ctx* c = new (std::nothrow) lsd_ctx();
    if (!c) return LSD_ERR_NOMEM;
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus;
    }
    {   // make_geom holds K1's window against this: without it no parameter set could be accepted or refused honestly
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || lds <= 0) { delete c; return LSD_ERR_HIP; }
        c->max_lds = (size_t)lds;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return LSD_ERR_HIP; }
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete c; return LSD_ERR_HIP; }
    if (hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming) != hipSuccess) { delete c; return LSD_ERR_HIP; }
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return LSD_ERR_HIP; }
    for (int k = 0; k < 2; k++)
        if (hipHostMalloc((void**)&c->pin[k], kPinBytes, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming) != hipSuccess) { delete c; return LSD_ERR_NOMEM; }
    c->last_stream = c->stream;
    // Schedule settings of the region stage.  The shipped library reads two from the environment, once, here: LSD_REGION_HELP (as
    // lsd_set_region_help) and LSD_REGION_POOL (calls with at most this many images get helper-only workgroups).  The others are
    // developer settings: lsd_debug_set_tuning() by name, and -- in the developer builds only (make stats / exp: -DLSD_DEVELOPER_KNOBS)
    // -- LSD_REGION_<NAME> from the environment.  None changes a result (tests/test_parity_gpu.py::
    // test_schedule_of_the_region_stage_changes_nothing); every value is clamped to the range the kernel assumes.
    for (const Tuning& t : kTunings) {
        const std::string name = std::string("LSD_REGION_") + t.name;
        const char* e = getenv(name.c_str());
        if (!e || !*e) continue;
#ifndef LSD_DEVELOPER_KNOBS
        if (!t.shipped) {                               // say so once: a sweep script that drives the shipped library by these would measure one configuration n times
            static bool warned = false;
            if (!warned) fprintf(stderr, "liblsdhip: %s is set but only read by the developer builds (make stats / exp, LSD_HIP_LIB=...); "
                                         "use lsd_debug_set_tuning() with the shipped library\n", name.c_str());
            warned = true;
            continue;
        }
#endif
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e) continue;
        c->*(t.field) = (int)(v < t.lo ? t.lo : v > t.hi ? t.hi : v);
    }
    *out = c;
    return LSD_OK;
}

void lsd_destroy(lsd_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    if (c->ga_ev) (void)hipEventDestroy(c->ga_ev);
    for (int k = 0; k < 2; k++) { if (c->pin[k]) (void)hipHostFree(c->pin[k]); if (c->pin_ev[k]) (void)hipEventDestroy(c->pin_ev[k]); }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                     // (every device buffer is a DevBuf member: freed here)
}

const char* lsd_last_error(const lsd_ctx* c) { return c ? c->err.c_str() : ""; }
void lsd_free(void* p) { free(p); }

int lsd_set_stop_after(lsd_ctx* c, int stage) {
    if (!c || stage < 0 || stage > LSD_STAGE_REGION) return LSD_ERR_INVALID;
    c->stop_after = stage;
    return LSD_OK;
}
int lsd_set_region_waves(lsd_ctx* c, int waves) {
    if (!c || (waves != 0 && waves != 4 && waves != 8)) return LSD_ERR_INVALID;
    c->region_waves_mode = waves;
    return LSD_OK;
}

int lsd_set_region_help(lsd_ctx* c, int waves) {
    if (!c || waves < -1 || waves > 4096) return LSD_ERR_INVALID;
    c->tun_help = waves;
    return LSD_OK;
}

int lsd_set_cost_history(lsd_ctx* c, int on) {
    if (!c) return LSD_ERR_INVALID;
    c->cost_history = on != 0;
    return LSD_OK;
}

int lsd_debug_set_tuning(lsd_ctx* c, const char* name, int value) {
    if (!c || !name) return LSD_ERR_INVALID;
    for (const Tuning& t : kTunings)
        if (strcmp(name, t.name) == 0) {
            c->*(t.field) = value < t.lo ? t.lo : value > t.hi ? t.hi : value;
            return LSD_OK;
        }
    return LSD_ERR_INVALID;
}

int lsd_debug_set_stamp_budget(lsd_ctx* c, unsigned grows) {
    if (!c || grows < 2u || grows > 0xFFFF0u) return LSD_ERR_INVALID;
    c->id_budget = grows;
    return LSD_OK;
}

// Test hook: every array the front end has to fill is set to 0xFF bytes (NaN doubles, words of all ones, a list length of -1) over its
// whole capacity, so that a store the next call leaves out shows in what lsd_debug_fetch returns instead of hiding behind the previous
// call's value at the same address.  The maxima and the near-tie counts are the call's own to clear and are left alone.
int lsd_debug_poison_front(lsd_ctx* c) {
    if (!c) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    Workspace& w = c->ws;
    auto fill = [&](void* p, size_t bytes) { return (p && bytes) ? hipMemset(p, 0xFF, bytes) : hipSuccess; };
    HIPCHK(c, fill(w.gauss.get(), w.gauss.capacity() * sizeof(double)));
    HIPCHK(c, fill(w.mag.get(), w.mag.capacity() * sizeof(double)));
    HIPCHK(c, fill(w.deg.get(), w.deg.capacity() * sizeof(double)));
    HIPCHK(c, fill(w.sc.get(), w.sc.capacity() * sizeof(double2)));
    HIPCHK(c, fill(w.pw.get(), w.pw.capacity() * sizeof(uint32_t)));
    HIPCHK(c, fill(w.ord.get(), w.ord.capacity() * sizeof(uint32_t)));
    HIPCHK(c, fill(w.nb.get(), w.nb.capacity() * sizeof(int32_t)));
    HIPCHK(c, hipDeviceSynchronize());
    return LSD_OK;
}

int lsd_set_trace(lsd_ctx* c, int on) {
    if (!c) return LSD_ERR_INVALID;
    c->trace = on != 0;
    return LSD_OK;
}

int lsd_set_fused_front(lsd_ctx* c, int on) {
    if (!c) return LSD_ERR_INVALID;
    c->fused_front = on != 0;
    return LSD_OK;
}

int lsd_set_fused_lines(lsd_ctx* c, int on) {
    if (!c) return LSD_ERR_INVALID;
    c->fused_lines = on != 0;
    return LSD_OK;
}

// The scan capacity: the largest stride the FeatureScan and ingest entries take.  1024 (k_rdp's static arrays) unless the caller asks
// for more; above it the launches go to k_rdp_long, whose LDS grows with the stride (k_rdp_lds.h): a capacity whose scans would not fit
// this device's LDS is refused here, before anything is enqueued -- make_geom's rule for K1's window.
int lsd_set_scan_capacity(lsd_ctx* c, int readings) {
    if (!c || readings < kRdpShortMaxLen) return LSD_ERR_INVALID;
    if (readings > LSD_SCAN_MAX_LEN) return LSD_ERR_UNSUPPORTED;
    if (readings > kRdpShortMaxLen && rdp_long_lds(readings) > c->max_lds) {
        char buf[200];
        snprintf(buf, sizeof buf, "scan capacity %d: FeatureScan's work arrays need %zu bytes of LDS, the device gives a workgroup %zu", readings,
                 rdp_long_lds(readings), c->max_lds);
        c->err = buf;
        return LSD_ERR_UNSUPPORTED;
    }
    if (readings != c->scan_cap) { c->scan_cap = readings; c->rdp_long_ready = false; }
    return LSD_OK;
}

int lsd_scan_capacity(const lsd_ctx* c) { return c ? c->scan_cap : LSD_ERR_INVALID; }

int lsd_reserve(lsd_ctx* c, int n, int cols, int rows) {
    if (!c || n <= 0) return LSD_ERR_INVALID;
    lsd_params p; lsd_default_params(&p);
    Geom g;
    int st = make_geom(c, &p, cols, rows, &g);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    st = ensure_workspace(c, (size_t)n, (size_t)g.npx, gauss_elems(c, g), c->ws.cap_max_lines, c->trace);
    if (st != LSD_OK) return st;
    // ... and the tables: the log-gamma table is sized by the geometry (w*h + 2 host-libm values: ~40 ms of host work and a blocking
    // copy for a 2048^2 map), taps / centres / log p for the default parameters.  Done here, the first enqueue after a reserve neither
    // allocates nor synchronises; ensure_tables' own grow path stays as the fallback for a LARGER geometry or other parameters later
    // (other parameters: three small blocking copies, no allocation).
    return ensure_tables(c, &p, g, nullptr);
}

int lsd_enqueue_batch_device(lsd_ctx* c, uint8_t* d_maps, int n, int cols, int rows, const lsd_params* p,
                             unsigned flags, uint8_t* d_line_ims, lsd_line* d_lines, int max_lines, int32_t* d_counts,
                             void* stream) {
    if (!c || !d_maps || n <= 0 || !d_lines || !d_counts || max_lines <= 0) return LSD_ERR_INVALID;
    Geom g;
    int st = make_geom(c, p, cols, rows, &g);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;              // NULL: the default (null) stream, as everywhere in HIP
    st = ensure_workspace(c, (size_t)n, (size_t)g.npx, gauss_elems(c, g), max_lines, c->trace);
    if (st != LSD_OK) return st;
    st = ensure_tables(c, p, g, s);
    if (st != LSD_OK) return st;
    const bool fused = use_front(c, g);
    if (!fused) HIPCHK(c, prepare_gauss(g));
    // the workspace is shared by every detector run of this context: one queued on another stream (done_stream: where ev_done was recorded)
    // must be over first
    if (c->done_valid && c->done_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_done, 0));

    Workspace& w = c->ws;
    Buffers b{};
    b.in = d_maps;
    b.in_rw = (flags & LSD_FLAG_WRITEBACK_MAP) ? d_maps : nullptr;
    b.gauss = w.gauss.get(); b.mag = w.mag.get(); b.deg = w.deg.get(); b.sc = w.sc.get(); b.pw = w.pw.get(); b.epochmap = w.epochmap.get(); b.sets = w.sets.get(); b.maxbits = w.maxbits.get(); b.nb = w.nb.get(); b.ties = w.ties();
    b.ord = w.ord.get(); b.spill = w.spill.get(); b.gcopy = w.gcopy.get(); b.wmeta = w.wmeta.get(); b.mcap = c->mcap; b.stamps = w.stamps.get(); b.seedidx = w.seedidx.get(); b.seedpos = w.seedpos.get(); b.tepoch = w.tepoch.get();
    b.tm_stride = 4 * ((g.w + 7) >> 3) * ((g.h + 7) >> 3);
    b.order = w.order.get(); b.slist = w.slist.get(); b.gcap = c->gcap; b.id_budget = c->id_budget; b.pend = w.pend.get(); b.rnum = w.rnum.get();
    b.recs = w.recs.get(); b.recs_scaled = w.recs_scaled.get(); b.counts = d_counts; b.lines = d_lines; b.line_im = d_line_ims;
    b.max_lines = max_lines;
    {   // the region stage's schedule (k_region.hip): look-ahead of the seed hand-out and of the full evaluations (seeds ahead of the
        // cursor; it adapts between the two values), idle lane groups per refill, results a wave may have waiting for the cursor
        const int nw = waves_for(c, n);
        b.tun_soft = c->tun_soft > 0 ? c->tun_soft : 48 * nw;
        b.tun_claim = c->tun_claim > 0 ? c->tun_claim : 192 * nw;
        b.tun_feed = c->tun_feed;
        b.tun_big = c->tun_big > 0 ? c->tun_big : 3;
        // Help across workgroups is OFF unless lsd_set_region_help asks for it (round 6).  Round 5 had already taken it away from calls of more
        // than 64 images (every image of a large batch pays for the protocol and few are helped: 512 maps 83 ms with, 78 without).  Since the
        // certified sets answer the structures that used to make single images heavy, it loses or ties everywhere else too
        // (profiles/r06q_help_small_probe.log, 2048^2 bench images, with / without): 1 image 8.9 / 8.9 ms, a heavy one 50.5 / 49.9; 2 heavy
        // images 59.2 / 49.7; 4: 55.9 / 48.5; 16: 39.1 / 37.2; 64: 51.4 / 50.2; the reference's maps one per call 1.01 / 0.96 ... 6.37 / 6.36 ms.
        b.tun_help = c->tun_help >= 0 ? c->tun_help : 0;
        b.tun_early = c->tun_early; b.tun_wb = c->tun_wb; b.tun_gate = c->tun_gate; b.tun_share = c->tun_share; b.tun_up = c->tun_up; b.tun_down = c->tun_down; b.tun_requeue = c->tun_requeue;
        b.tun_xpoll = c->tun_xpoll; b.tun_linger = c->tun_linger; b.tun_stop = c->tun_stop;
        b.xq = (b.tun_help > 0 && !c->trace) ? w.xq.get() : nullptr;
        b.npool = b.xq ? pool_for(c, n) : 0;
    }
    b.taps = c->d_taps.get(); b.centres = c->d_centres.get(); b.lgamma = c->d_lgamma.get(); b.lg_count = (int)c->d_lgamma.capacity(); b.ptab = c->d_ptab.get();
    b.seeds = c->trace ? w.seeds.get() : nullptr; b.nseed = w.nseed.get(); b.stats = w.stats.get();

    // Every dispatch of a batch in flight has to get onto a hardware pipe that the launches of other batches may be holding (a region launch
    // waits for workgroup slots for tens of milliseconds), so a batch costs as few dispatches as it can: ONE fill in front of the kernels (the
    // gradient maxima and, behind them, the gradient pass's near-tie counts); the region stage clears its own counter records and tile epochs
    // image by image; the line counts and list lengths are written by the kernels that own them unless the pipeline is cut short; an image's
    // lines are written by the region stage's workgroup that finished it (fused_lines) -- not behind a seed trace, not with help across
    // workgroups (the owner's wavefronts go on to help others: they do not meet at the image's end), not where stop_after cuts the lines off.
    b.fuse_lines = (c->fused_lines && c->stop_after == 0 && !c->trace && !b.xq) ? 1 : 0;
    HIPCHK(c, hipMemsetAsync(w.maxbits.get(), 0, sizeof(unsigned long long) * w.cap_n + sizeof(int32_t) * (size_t)n, s));
    const bool full_region = c->stop_after == 0 || c->stop_after >= LSD_STAGE_REGION;
    if (!full_region) HIPCHK(c, hipMemsetAsync(d_counts, 0, sizeof(int32_t) * n, s));            // (else k_region writes every image's count)
    if (c->stop_after != 0 && c->stop_after < LSD_STAGE_SORT) HIPCHK(c, hipMemsetAsync(w.nb.get(), 0, sizeof(int32_t) * (size_t)n, s));   // (else k_sort writes every image's length)

    HIPCHK(c, hipEventRecord(c->ev[0], s));
    // Mat::zeros, myLSD.cpp:215: the Gaussian's tiles clear lineIm on the way where the raster is made of whole 16-byte words; else a
    // kernel of its own does (inside the event window either way: part of "gauss")
    const bool fused_clear = d_line_ims && (((size_t)cols * rows) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_line_ims) & 15) == 0;
    if (d_line_ims && !fused_clear) launch_clear(d_line_ims, (size_t)n * cols * rows, c->num_cus, s);
    // K1 and K2 as one kernel where that applies (use_front): its time is reported under "gauss" and "gradient" reads exactly 0
    // (lsd_last_timings) -- two events back to back would give microseconds
    if (fused) launch_front(g, b, n, fused_clear ? d_line_ims : nullptr, s);
    else launch_gauss(g, b, n, fused_clear ? d_line_ims : nullptr, false, s);
    if (b.in_rw) launch_remap_writeback(g, b, n, s);
    HIPCHK(c, hipEventRecord(c->ev[1], s));
    if (!fused && (c->stop_after == 0 || c->stop_after >= LSD_STAGE_GRAD)) launch_gradient(g, b, n, s);
    HIPCHK(c, hipEventRecord(c->ev[2], s));
    if (c->stop_after == 0 || c->stop_after >= LSD_STAGE_SORT) { launch_sort(g, b, n, s); launch_order(b, n, g.npx, (c->cost_history && c->hist_n == n && !c->trace) ? w.stats.get() : nullptr, s); }
    HIPCHK(c, hipEventRecord(c->ev[3], s));
    hipStream_t sr = s;
    if (c->stop_after == 0 || c->stop_after >= LSD_STAGE_REGION) {
        // stamps of earlier runs must never look current: every run gets its own 2^20-wide id range
        if (++w.run_id >= 1023u) {
            HIPCHK(c, hipMemsetAsync(w.stamps.get(), 0, w.cap_ws * tm_words(w.cap_npx) * sizeof(uint32_t), sr));
            HIPCHK(c, hipMemsetAsync(w.epochmap.get(), 0, w.cap_n * w.cap_npx * sizeof(uint32_t), sr));   // (the set labels carry the run number too)
            w.run_id = 1;
        }
        // (the counter records and the tile epochs are cleared by the region stage itself, image by image: region_image)
        if (b.xq) HIPCHK(c, hipMemsetAsync(b.xq, 0, sizeof(uint32_t) * ((size_t)n * (kXStride + 1) + kXHdr), sr));
        // 8 wavefronts per image take a whole CU each: worth it up to four images per CU (waves_for); the per-wave workspace
        // (stamps / spill / gcopy: 12 B per scaled pixel and wave) was sized for it by ensure_workspace
        const bool wide = waves_for(c, n) == 8;
        int grid = n;
        const int groups = c->tun_groups >= 0 ? c->tun_groups : c->num_cus;
        if (wide && groups > 0 && groups < n && !b.xq && !c->trace) {           // persistent workgroups (k_region.hip: k_region): fewer workgroups than images
            if (!c->pcount.get()) HIPCHK(c, c->pcount.resize(16));
            HIPCHK(c, hipMemsetAsync(c->pcount.get(), 0, sizeof(int), sr));
            b.pcount = c->pcount.get(); b.nimg = n; b.npool = 0;
            grid = groups;
        }
        if (wide) launch_region_w8(g, b, grid, w.run_id << 20, sr);
        else launch_region_w4(g, b, grid, w.run_id << 20, sr);
    }
    HIPCHK(c, hipEventRecord(c->ev[4], s));
    if (c->stop_after == 0 && !b.fuse_lines) launch_lines(g, b, n, s);
    HIPCHK(c, hipEventRecord(c->ev[5], s));
    HIPCHK(c, hipEventRecord(c->ev_done, s));
    c->done_valid = true; c->done_stream = s;
    HIPCHK(c, hipGetLastError());
    c->ev_valid = true;
    c->hist_n = (c->stop_after == 0 || c->stop_after >= LSD_STAGE_REGION) ? n : 0;     // (the counter records of this launch: the next one's cost history)
    c->geom = g; c->last_n = n; c->last_max_lines = max_lines; c->last_counts = d_counts; c->last_stream = s;
    c->last_fused = fused; c->last_in = d_maps; c->last_remapped = b.in_rw != nullptr;
    c->last_lines_fused = b.fuse_lines != 0;
    return LSD_OK;
}

int lsd_synchronize(lsd_ctx* c) {
    if (!c) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    return LSD_OK;
}

int lsd_last_timings(lsd_ctx* c, float ms[6]) {
    if (!c || !ms || !c->ev_valid) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev[5]));
    for (int i = 0; i < 5; i++) HIPCHK(c, hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    HIPCHK(c, hipEventElapsedTime(&ms[5], c->ev[0], c->ev[5]));
    if (c->last_fused) ms[1] = 0.0f;                                 // (the fused front end: all of it is under "gauss")
    if (c->last_lines_fused) ms[4] = 0.0f;                           // (... and the lines written by the region stage under "region")
    return LSD_OK;
}

// Host -> device through the two pinned buffers: the memcpy into one overlaps the DMA out of the other.
static int h2d_staged(lsd_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t s) {
    size_t off = 0;
    for (int k = 0; off < bytes; k++) {
        const int b = k & 1;
        const size_t len = bytes - off < kPinBytes ? bytes - off : kPinBytes;
        if (c->pin_used[b]) HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));   // (also a DMA left behind by a call that returned with an error)
        memcpy(c->pin[b], (const uint8_t*)src + off, len);
        HIPCHK(c, hipMemcpyAsync((uint8_t*)dst + off, c->pin[b], len, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->pin_ev[b], s));
        c->pin_used[b] = true;
        off += len;
    }
    return LSD_OK;
}
// Device -> host the same way (returns when the bytes are in dst).
static int d2h_staged(lsd_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t s) {
    size_t off = 0, prev_off = 0, prev_len = 0;
    for (int k = 0; off < bytes; k++) {
        const int b = k & 1;
        const size_t len = bytes - off < kPinBytes ? bytes - off : kPinBytes;
        if (c->pin_used[b] && k < 2) HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));
        HIPCHK(c, hipMemcpyAsync(c->pin[b], (const uint8_t*)src + off, len, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->pin_ev[b], s));
        c->pin_used[b] = true;
        if (prev_len) {
            HIPCHK(c, hipEventSynchronize(c->pin_ev[b ^ 1]));
            memcpy((uint8_t*)dst + prev_off, c->pin[b ^ 1], prev_len);
        }
        prev_off = off; prev_len = len;
        off += len;
        if (off >= bytes) {
            HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));
            memcpy((uint8_t*)dst + prev_off, c->pin[b], prev_len);
        }
    }
    return LSD_OK;
}

static int ensure_host_staging(lsd_ctx* c, size_t n, size_t wh, int max_lines, bool lineim) {
    if (n > c->hcap_n || wh > c->hcap_wh || max_lines > c->hcap_max_lines || (lineim && !c->hcap_lineim)) {
        const size_t nn = n > c->hcap_n ? n : c->hcap_n, ww = wh > c->hcap_wh ? wh : c->hcap_wh;
        const int ml = max_lines > c->hcap_max_lines ? max_lines : c->hcap_max_lines;
        const bool li = lineim || c->hcap_lineim;
        c->hcap_n = 0; c->hcap_wh = 0; c->hcap_max_lines = 0; c->hcap_lineim = false;   // (stay 0 if an allocation below fails)
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, c->h_in.resize(nn * ww));
        HIPCHK(c, c->h_lineim.resize(li ? nn * ww : 0));
        HIPCHK(c, c->h_lines.resize(nn * (size_t)ml)); HIPCHK(c, c->h_flat.resize(nn * (size_t)ml));
        HIPCHK(c, c->h_counts.resize(nn)); HIPCHK(c, c->h_offs.resize(nn + 3));
        c->hcap_n = nn; c->hcap_wh = ww; c->hcap_max_lines = ml; c->hcap_lineim = li;
    }
    return LSD_OK;
}

int lsd_run_batch(lsd_ctx* c, uint8_t* maps, int n, int cols, int rows, const lsd_params* p, uint8_t* line_ims,
                  lsd_line** lines_out, int* offsets_out) {
    if (!c || !maps || n <= 0 || !lines_out || !offsets_out) return LSD_ERR_INVALID;
    *lines_out = nullptr;
    Geom g;
    int st = make_geom(c, p, cols, rows, &g);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t wh = (size_t)cols * rows;
    const int ml = c->host_max_lines;
    if ((long long)n * ml >= (1ll << 31) / 10) return LSD_ERR_UNSUPPORTED;   // (int32 offsets into the flat record array)
    st = ensure_host_staging(c, (size_t)n, wh, ml, line_ims != nullptr);
    if (st != LSD_OK) return st;
    hipStream_t s = c->stream;
    st = h2d_staged(c, c->h_in.get(), maps, (size_t)n * wh, s);
    if (st != LSD_OK) return st;
    st = lsd_enqueue_batch_device(c, c->h_in.get(), n, cols, rows, p, LSD_FLAG_WRITEBACK_MAP, line_ims ? c->h_lineim.get() : nullptr,
                                  c->h_lines.get(), ml, c->h_counts.get(), s);
    if (st != LSD_OK) return st;
    launch_compact_lines(c->h_lines.get(), c->h_counts.get(), ml, n, c->h_flat.get(), c->h_offs.get(), s);
    // the observable in-place remap is final after K1 (event 1 of the enqueue): it travels back on the second stream while
    // the gradient / sort / region / line kernels run
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev[1], 0));
    st = d2h_staged(c, maps, c->h_in.get(), (size_t)n * wh, c->copy_stream);
    if (st != LSD_OK) return st;
    std::vector<int32_t> offs((size_t)n + 3);                                                  // offsets[n + 1], the overflow count, 1 + first image given up
    st = d2h_staged(c, offs.data(), c->h_offs.get(), sizeof(int32_t) * (size_t)(n + 3), s);          // (waits for the pipeline)
    if (st != LSD_OK) return st;
    memcpy(offsets_out, offs.data(), sizeof(int32_t) * (size_t)(n + 1));
    const int total = offsets_out[n];
    lsd_line* out = (lsd_line*)calloc(total > 0 ? total : 1, sizeof(lsd_line));
    if (!out) return LSD_ERR_NOMEM;
    st = total > 0 ? d2h_staged(c, out, c->h_flat.get(), sizeof(lsd_line) * (size_t)total, s) : LSD_OK;
    if (st == LSD_OK && line_ims) st = d2h_staged(c, line_ims, c->h_lineim.get(), (size_t)n * wh, s);
    if (st != LSD_OK) { free(out); return st; }
    *lines_out = out;
    if (offs[(size_t)n + 2] > 0) {
        // the region stage's watchdog gave an image up (a defect of its protocol, never seen on a released build): that image has
        // no lines in the result, everything else is valid
        c->err = "region stage gave up image " + std::to_string(offs[(size_t)n + 2] - 1) + " of the batch (watchdog; counts = -1)";
        return LSD_ERR_INTERNAL;
    }
    // more lines than host_max_lines in some image: the first host_max_lines of it are returned, and the status says so
    return offs[(size_t)n + 1] > 0 ? LSD_ERR_CAPACITY : LSD_OK;
}

int lsd_set_host_max_lines(lsd_ctx* c, int max_lines) {
    if (!c || max_lines < 1 || max_lines > (1 << 20)) return LSD_ERR_INVALID;
    c->host_max_lines = max_lines;
    return LSD_OK;
}

int lsd_run(lsd_ctx* c, uint8_t* map, int cols, int rows, size_t stride, const lsd_params* p, uint8_t* line_im,
            size_t line_im_stride, lsd_line** lines_out, int* n_lines) {
    if (!c || !map || !lines_out || !n_lines || cols <= 0 || rows <= 0) return LSD_ERR_INVALID;
    if (stride < (size_t)cols || (line_im && line_im_stride < (size_t)cols)) return LSD_ERR_INVALID;
    *n_lines = 0;
    const bool packed = stride == (size_t)cols && (!line_im || line_im_stride == (size_t)cols);
    int offs[2] = {0, 0};
    if (packed) {
        int st = lsd_run_batch(c, map, 1, cols, rows, p, line_im, lines_out, offs);
        *n_lines = offs[1];
        return st;
    }
    std::vector<uint8_t> tmp((size_t)cols * rows), tim(line_im ? (size_t)cols * rows : 0);
    for (int y = 0; y < rows; y++) memcpy(&tmp[(size_t)y * cols], map + (size_t)y * stride, cols);
    int st = lsd_run_batch(c, tmp.data(), 1, cols, rows, p, line_im ? tim.data() : nullptr, lines_out, offs);
    for (int y = 0; y < rows; y++) memcpy(map + (size_t)y * stride, &tmp[(size_t)y * cols], cols);
    if (line_im)
        for (int y = 0; y < rows; y++) memcpy(line_im + (size_t)y * line_im_stride, &tim[(size_t)y * cols], cols);
    *n_lines = offs[1];
    return st;
}

int lsd_last_region_cycles(lsd_ctx* c, int n, long long* cycles_out) {
    // (hist_n: images of the last call whose REGION stage ran -- 0 after a call that lsd_set_stop_after ended earlier, whose counter
    //  records would be stale or zero)
    if (!c || !cycles_out || n <= 0 || n > c->last_n || n > c->hist_n) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy2D(cycles_out, sizeof(long long), c->ws.stats.get() + kStatTotalWord, sizeof(long long) * kStatWords, sizeof(long long), (size_t)n,
                          hipMemcpyDeviceToHost));
    return LSD_OK;
}

int lsd_last_sensitivity(lsd_ctx* c, int n, int* near_ties) {
    if (!c || !near_ties || n <= 0 || n > c->last_n || n > c->hist_n) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    std::vector<long long> reg((size_t)n);
    std::vector<int32_t> grad((size_t)n);
    HIPCHK(c, hipMemcpy2D(reg.data(), sizeof(long long), c->ws.stats.get() + kStatTiesWord, sizeof(long long) * kStatWords, sizeof(long long), (size_t)n,
                          hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(grad.data(), c->ws.ties(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        const long long v = reg[(size_t)i] + grad[(size_t)i];
        near_ties[i] = v > 0x7fffffffll ? 0x7fffffff : (int)v;
    }
    return LSD_OK;
}

int lsd_debug_fetch(lsd_ctx* c, int image, int what, void* out, size_t bytes) {
    if (!c || !out || image < 0 || image >= c->last_n) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    const Workspace& w = c->ws;
    const size_t npx = (size_t)c->geom.npx, off = (size_t)image * npx;
    const void* src = nullptr;
    size_t need = 0;
    int32_t nbv = 0, cnt = 0, nseed = 0;
    switch (what) {
        case LSD_DBG_GAUSS:                                           // (rows are padded to gp doubles on the device)
            if (bytes < npx * 8) return LSD_ERR_INVALID;
            if (c->last_fused) {
                // no Gaussian image exists after the fused front end: K1 alone computes the requested one from the call's input (still
                // alive: lsd_hip.h), without the remap where the call has rewritten that input in place since (not idempotent: 1 -> 255 -> 0)
                const Geom& g = c->geom;
                HIPCHK(c, c->dbg_gauss.reserve((size_t)g.gp * g.h));
                HIPCHK(c, prepare_gauss(g));
                Buffers b{};
                b.in = c->last_in + (size_t)image * g.W * g.H; b.gauss = c->dbg_gauss.get();
                b.taps = c->d_taps.get(); b.centres = c->d_centres.get();
                launch_gauss(g, b, 1, nullptr, c->last_remapped, c->last_stream);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipStreamSynchronize(c->last_stream));
                HIPCHK(c, hipMemcpy2D(out, (size_t)g.w * 8, c->dbg_gauss.get(), (size_t)g.gp * 8, (size_t)g.w * 8, (size_t)g.h, hipMemcpyDeviceToHost));
                return LSD_OK;
            }
            HIPCHK(c, hipMemcpy2D(out, (size_t)c->geom.w * 8, w.gauss.get() + (size_t)image * c->geom.gp * c->geom.h, (size_t)c->geom.gp * 8,
                                  (size_t)c->geom.w * 8, (size_t)c->geom.h, hipMemcpyDeviceToHost));
            return LSD_OK;
        case LSD_DBG_MAG: src = w.mag.get() + off; need = npx * 8; break;
        case LSD_DBG_DEG: src = w.deg.get() + off; need = npx * 8; break;
        case LSD_DBG_STATE: src = w.pw.get() + off; need = npx * 4; break;
        case LSD_DBG_ORDER:
        case LSD_DBG_ORDER_VAL:
            HIPCHK(c, hipMemcpy(&nbv, w.nb.get() + image, 4, hipMemcpyDeviceToHost));
            if (what == LSD_DBG_ORDER) { src = w.ord.get() + off; need = (size_t)nbv * 4; }
            else {                                                    // the bin values are recomputed on demand (k_sort.hip: k_ordv)
                if (bytes < (size_t)nbv * 2) return LSD_ERR_INVALID;
                DevBuf<uint16_t> tmp;
                HIPCHK(c, tmp.resize((size_t)(nbv > 0 ? nbv : 1)));
                launch_ordv(w.mag.get() + off, w.maxbits.get() + image, w.ord.get() + off, tmp.get(), nbv, c->geom.pseBin, c->last_stream);
                HIPCHK(c, hipStreamSynchronize(c->last_stream));
                if (nbv > 0) HIPCHK(c, hipMemcpy(out, tmp.get(), (size_t)nbv * 2, hipMemcpyDeviceToHost));
                return LSD_OK;
            }
            break;
        case LSD_DBG_NB: src = w.nb.get() + image; need = 4; break;
        case LSD_DBG_MAXGRAD: src = w.maxbits.get() + image; need = 8; break;
        case LSD_DBG_RECS:
            HIPCHK(c, hipMemcpy(&cnt, c->last_counts + image, 4, hipMemcpyDeviceToHost));
            if (cnt > c->last_max_lines) cnt = c->last_max_lines;
            src = w.recs.get() + (size_t)image * c->last_max_lines * 12; need = (size_t)cnt * 12 * 8;
            break;
        case LSD_DBG_NSEED: src = w.nseed.get() + image; need = 4; break;
        case LSD_DBG_SEEDS:
            if (!w.seeds.get()) return LSD_ERR_INVALID;
            HIPCHK(c, hipMemcpy(&nseed, w.nseed.get() + image, 4, hipMemcpyDeviceToHost));
            src = w.seeds.get() + off; need = (size_t)nseed * sizeof(SeedRec);
            break;
        case LSD_DBG_STATS:                                           // (a larger `bytes` reads the records of the following images too)
            src = w.stats.get() + (size_t)image * kStatWords; need = 8 * kStatWords;
            if (bytes > need) { const size_t all = (size_t)(c->last_n - image) * need; need = bytes < all ? bytes / need * need : all; }
            break;
        case LSD_DBG_SINCOS: src = w.sc.get() + off; need = npx * 16; break;      // (defined where the pixel's code is 0: lsd_hip.h)
        case LSD_DBG_PW: src = w.pw.get() + off; need = npx * 4; break;           // (STATE without the reduction to usedMap below)
        case LSD_DBG_GRAD_TIES: src = w.ties() + image; need = 4; break;
        default: return LSD_ERR_INVALID;
    }
    if (bytes < need) return LSD_ERR_INVALID;
    if (need) HIPCHK(c, hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    if (what == LSD_DBG_STATE) {                                   // packed pixel words -> usedMap values (lsd_internal.h)
        uint32_t* o = static_cast<uint32_t*>(out);
        for (size_t i = 0; i < npx; i++) o[i] = pw_used(o[i]);
    }
    return LSD_OK;
}

// createMapCache's scratch for n maps of `cells` cells (lsd_enqueue_map_cache_device): grow-only, nothing happens while it suffices
static int reserve_map_cache(lsd_ctx* c, size_t n, size_t cells) {
    const size_t need = n * cells;
    HIPCHK(c, c->mc_claim.reserve(need)); HIPCHK(c, c->mc_fa.reserve(need * 2)); HIPCHK(c, c->mc_fb.reserve(need * 2));
    HIPCHK(c, c->mc_ctl.reserve(n * (2 + 64)));                                        // frontier sizes + up to 64 chunk counts per map
    return LSD_OK;
}

int lsd_enqueue_map_cache_device(lsd_ctx* c, const uint8_t* d_maps, int n, int cols, int rows, double res,
                                 double z_occ_max_dis, double* d_out, void* stream) {
    if (!c || !d_maps || !d_out || n <= 0 || cols <= 0 || rows <= 0 || !(res > 0) || !(z_occ_max_dis >= 0)) return LSD_ERR_INVALID;
    if ((long long)cols * rows >= (1ll << 31)) return LSD_ERR_UNSUPPORTED;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;              // NULL: the default (null) stream, as everywhere in HIP
    const int rs = reserve_map_cache(c, (size_t)n, (size_t)cols * rows);
    if (rs != LSD_OK) return rs;
    const int cell_radius = cvt_x86(floor(z_occ_max_dis / res));           // myLSD.cpp:13
    // few maps: spread each over G workgroups (kernel per level phase); many maps: one workgroup per map, one launch
    int G = (2 * c->num_cus) / n;
    if (G > 64) G = 64;
    if (G >= 4)                                                    // measured crossover: 128 maps 33 vs 42 ms, 256 maps 67 vs 56 ms
        launch_mapcache_spread(d_maps, d_out, c->mc_claim.get(), c->mc_fa.get(), c->mc_fb.get(), c->mc_ctl.get(), c->mc_ctl.get() + 2 * (size_t)n, n, G, cols, rows, res,
                               z_occ_max_dis, cell_radius, s);
    else
        launch_mapcache(d_maps, d_out, c->mc_claim.get(), c->mc_fa.get(), c->mc_fb.get(), n, cols, rows, res, z_occ_max_dis, cell_radius, s);
    HIPCHK(c, hipGetLastError());
    c->last_stream = s;
    return LSD_OK;
}

int lsd_map_cache(lsd_ctx* c, const uint8_t* map, int cols, int rows, size_t stride, double res, double z_occ_max_dis,
                  double* out) {
    if (!c || !map || !out || cols <= 0 || rows <= 0 || stride < (size_t)cols) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t wh = (size_t)cols * rows;
    HIPCHK(c, c->mc_in.reserve(wh)); HIPCHK(c, c->mc_out.reserve(wh));
    int st;
    if (stride == (size_t)cols) { st = h2d_staged(c, c->mc_in.get(), map, wh, c->stream); if (st != LSD_OK) return st; }
    else HIPCHK(c, hipMemcpy2DAsync(c->mc_in.get(), cols, map, stride, cols, rows, hipMemcpyHostToDevice, c->stream));
    st = lsd_enqueue_map_cache_device(c, c->mc_in.get(), 1, cols, rows, res, z_occ_max_dis, c->mc_out.get(), c->stream);
    if (st != LSD_OK) return st;
    return d2h_staged(c, out, c->mc_out.get(), wh * sizeof(double), c->stream);
}

int lsd_enqueue_occupancy_to_map_device(lsd_ctx* c, const int8_t* d_grid, size_t n_cells, uint8_t* d_map, void* stream) {
    if (!c || !d_grid || !d_map || n_cells == 0) return LSD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_grid) | reinterpret_cast<uintptr_t>(d_map)) & 15u) return LSD_ERR_INVALID;   // 16-byte accesses
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;              // NULL: the default (null) stream, as everywhere in HIP
    launch_occ_to_map(reinterpret_cast<const uint8_t*>(d_grid), d_map, n_cells, s);
    HIPCHK(c, hipGetLastError());
    c->last_stream = s;
    return LSD_OK;
}

int lsd_occupancy_to_map(lsd_ctx* c, const int8_t* grid, int cols, int rows, uint8_t* map_out, size_t map_stride) {
    if (!c || !grid || !map_out || cols <= 0 || rows <= 0 || map_stride < (size_t)cols) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t wh = (size_t)cols * rows;
    HIPCHK(c, c->oc_in.reserve(wh)); HIPCHK(c, c->oc_out.reserve(wh));
    HIPCHK(c, hipMemcpyAsync(c->oc_in.get(), grid, wh, hipMemcpyHostToDevice, c->stream));
    const int st = lsd_enqueue_occupancy_to_map_device(c, reinterpret_cast<const int8_t*>(c->oc_in.get()), wh, c->oc_out.get(), c->stream);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipMemcpy2DAsync(map_out, map_stride, c->oc_out.get(), cols, cols, rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LSD_OK;
}

int lsd_reserve_map_update(lsd_ctx* c, int cols, int rows) {
    if (!c || cols <= 0 || rows <= 0) return LSD_ERR_INVALID;
    if ((long long)cols * rows >= (1ll << 31)) return LSD_ERR_UNSUPPORTED;
    int st = lsd_reserve(c, 1, cols, rows);                         // the detector's workspace and the tables of the default parameters
    if (st != LSD_OK) return st;
    // ... its record arrays for as many lines per map as the host entry points take (lsd_set_host_max_lines: 128 B each), which
    // lsd_reserve leaves to the first enqueue because it is not told a capacity
    Geom g;
    lsd_params p; lsd_default_params(&p);
    st = make_geom(c, &p, cols, rows, &g);
    if (st != LSD_OK) return st;
    st = ensure_workspace(c, 1, (size_t)g.npx, gauss_elems(c, g), std::max(c->ws.cap_max_lines, c->host_max_lines), c->trace);
    if (st != LSD_OK) return st;
    return reserve_map_cache(c, 1, (size_t)cols * rows);
}

int lsd_enqueue_map_update_device(lsd_ctx* c, const int8_t* d_grid, int cols, int rows, double res, double z_occ_max_dis, const lsd_params* p,
                                  uint8_t* d_map, double* d_map_cache, lsd_line* d_lines, int max_lines, int32_t* d_count, uint8_t* d_line_im,
                                  void* stream) {
    // every refusal of the three entries below, taken here: nothing is enqueued unless all of them accept
    if (!c || !d_grid || !d_map || !d_map_cache || !d_lines || !d_count || max_lines <= 0 || cols <= 0 || rows <= 0 || !(res > 0) ||
        !(z_occ_max_dis >= 0))
        return LSD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_grid) | reinterpret_cast<uintptr_t>(d_map)) & 15u) {
        c->err = "map update: d_grid and d_map must be 16-byte aligned";
        return LSD_ERR_INVALID;
    }
    if ((long long)cols * rows >= (1ll << 31)) return LSD_ERR_UNSUPPORTED;
    Geom g;
    int st = make_geom(c, p, cols, rows, &g);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // The detector's workspace and createMapCache's scratch are the context's: an update on another stream than the last detector run's
    // goes behind the event that run recorded (an update ends with the detector, so the event covers its flood as well).
    if (c->done_valid && c->done_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_done, 0));
    const size_t cells = (size_t)cols * rows;
    st = lsd_enqueue_occupancy_to_map_device(c, d_grid, cells, d_map, s);                                  // main_on_linux.cpp:108-124
    if (st != LSD_OK) return st;
    st = lsd_enqueue_map_cache_device(c, d_map, 1, cols, rows, res, z_occ_max_dis, d_map_cache, s);        // :130, before the detector rewrites the map
    if (st != LSD_OK) return st;
    return lsd_enqueue_batch_device(c, d_map, 1, cols, rows, p, LSD_FLAG_WRITEBACK_MAP, d_line_im, d_lines, max_lines, d_count, s);   // :132
}

int lsd_debug_calibrate(lsd_ctx* c, size_t bytes) {
    if (!c || bytes < 8) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> buf;
    HIPCHK(c, buf.resize(bytes / 8));
    launch_calib(buf.get(), bytes / 8, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LSD_OK;
}

int lsd_debug_eval_math(lsd_ctx* c, int fn, const double* a, const double* b, double* out0, double* out1, size_t n) {
    if (!c || !a || !out0 || !out1 || n == 0 || fn < 0 || fn > 6 || ((fn == 1 || fn == 6) && !b)) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> da, db, d0, d1;
    HIPCHK(c, da.resize(n)); HIPCHK(c, db.resize(n)); HIPCHK(c, d0.resize(n)); HIPCHK(c, d1.resize(n));
    HIPCHK(c, hipMemcpy(da.get(), a, n * 8, hipMemcpyHostToDevice));
    if (b) HIPCHK(c, hipMemcpy(db.get(), b, n * 8, hipMemcpyHostToDevice));
    launch_dbgmath(fn, da.get(), db.get(), d0.get(), d1.get(), n, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out0, d0.get(), n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out1, d1.get(), n * 8, hipMemcpyDeviceToHost));
    return LSD_OK;
}

int lsd_debug_lines(lsd_ctx* c, const double* recs, int n, int cols, int rows, lsd_line* lines_out, uint8_t* line_im) {
    if (!c || !recs || !lines_out || n <= 0 || cols <= 0 || rows <= 0) return LSD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> dr; DevBuf<int32_t> dn; DevBuf<lsd_line> dl; DevBuf<uint8_t> di;
    const size_t px = (size_t)cols * rows;
    HIPCHK(c, dr.resize((size_t)n * 4)); HIPCHK(c, dn.resize(1)); HIPCHK(c, dl.resize(n));
    if (line_im) HIPCHK(c, di.resize(px));
    HIPCHK(c, hipMemcpy(dr.get(), recs, (size_t)n * 4 * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn.get(), &n, 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(dl.get(), 0xFF, (size_t)n * sizeof(lsd_line), c->stream));   // what K5 leaves unwritten shows
    if (line_im) launch_clear(di.get(), px, c->num_cus, c->stream);
    launch_lines_of(dr.get(), dn.get(), dl.get(), line_im ? di.get() : nullptr, n, cols, rows, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(lines_out, dl.get(), (size_t)n * sizeof(lsd_line), hipMemcpyDeviceToHost));
    if (line_im) HIPCHK(c, hipMemcpy(line_im, di.get(), px, hipMemcpyDeviceToHost));
    return LSD_OK;
}

}  // extern "C"
