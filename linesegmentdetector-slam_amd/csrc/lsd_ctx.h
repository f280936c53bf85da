// lsd_ctx.h -- the context of liblsdhip.so as the host files see it (lsd_ctx.hip: the context, the detector, the map cache and the map
// update; lsd_loc.hip: localisation -- scan matching, FeatureScan, FeatureAssociation, the carries and the replay loop; lsd_grid.hip: the
// grid stack; lsd_pg.hip: the pose graph; lsd_dist.hip: the hand-off between GPUs): the struct, the status macro, the tail every enqueue
// entry ends with and the round trip through the staging arena every host convenience makes.  Nothing here depends on
// LSD_DEVELOPER_KNOBS: the developer build's lsd_ctx_dev.o and every other object have to agree on the struct's layout.
#pragma once
#include <string>
#include <vector>

#include "lsd_devbuf.h"
#include "lsd_internal.h"
#include "k_rdp_lds.h"

using namespace lsdhip;   // (lsd_ctx is the C ABI's opaque type: it lives outside the namespace its members come from)

// The main workspace: everything ensure_workspace sizes from the batch geometry, with the capacities it was sized for.  A failed
// (re)allocation forgets all of it at once (`ws = Workspace{}`).
struct Workspace {
    size_t cap_gpx = 0;                          // Gaussian elements per image (rows padded to Geom::gp)
    size_t cap_n = 0, cap_npx = 0, cap_ws = 0;   // images, scaled pixels per image, wave slots
    int cap_max_lines = 0;
    DevBuf<double> gauss, mag, deg, recs, recs_scaled;
    DevBuf<double2> sc;
    DevBuf<uint32_t> order;
    DevBuf<uint32_t> sets;               // n x 256: certified sets of the region stage (region/eval.h: certify_set)
    DevBuf<uint32_t> pw, epochmap, ord, spill, gcopy, stamps, seedidx, seedpos, tepoch;
    uint32_t run_id = 0;   // curMap stamps are unique per run: (run_id << 20) + grow number (a wave that uses up its 2^20 clears its stamps)
    DevBuf<uint32_t> slist;
    DevBuf<double> pend;
    DevBuf<float4> wmeta;
    DevBuf<int> rnum;
    DevBuf<uint32_t> xq;
    DevBuf<unsigned long long> maxbits;  // [0, cap_n) the maxima, then cap_n int32: the gradient pass's near-tie counts -- one memset clears both
    DevBuf<int32_t> nb, nseed;
    DevBuf<long long> stats;
    DevBuf<SeedRec> seeds;               // allocated only while tracing is on
    int32_t* ties() const { return reinterpret_cast<int32_t*>(maxbits.get() + cap_n); }
};

struct lsd_ctx {
    int device = 0;
    int num_cus = 256;                 // compute units of the device
    size_t max_lds = 0;                // LDS a workgroup may have (hipDeviceAttributeMaxSharedMemoryPerBlock): bounds K1's window (make_geom)
    uint32_t id_budget = 0xFFFF0u;     // curMap stamp ids a wave may use per run before it clears its stamps (lsd_debug_set_stamp_budget)
    int tun_soft = 0, tun_claim = 0, tun_feed = 3, tun_big = 0;   // region-stage schedule (0: default), see k_region.hip
    int tun_help = -1;                                             // helper wavefronts per image (-1: default, 0: none)
    // developer experiments (environment variables read once, when the context is created; DESIGN_NOTES.md says what each was for)
    int tun_gate = 12000;                                          // an image asks for help once it has run for this long (x 1024 clocks: ~5 ms)
    int tun_share = 0;                                             // ... and for at least this share (%) of the time since the launch began (LSD_REGION_SHARE)
    int pool_max_images = 4;                                       // calls with at most this many images get a pool of helper workgroups (LSD_REGION_POOL)
    int tun_early = 0, tun_wb = 10, tun_up = 32, tun_down = 96, tun_requeue = 1, tun_xpoll = 20000, tun_linger = 1000000, tun_stop = 0;
    int region_waves_mode = 0;         // 0: choose per batch; 4 / 8: force that region-stage variant (lsd_set_region_waves)
    bool prefer4 = false;              // the 8-wave workspace did not fit this device's memory once: batches run on 4 waves per image
    hipStream_t stream = nullptr;      // the context's own stream
    hipStream_t last_stream = nullptr; // stream of the last enqueue
    std::string err;
    Workspace ws;
    int mcap = 16384;
    int gcap = 8192;
    // host-API staging (device side), and the pinned host buffers every host <-> device copy goes through
    DevBuf<uint8_t> h_in, h_lineim;
    DevBuf<lsd_line> h_lines, h_flat;
    DevBuf<int32_t> h_counts, h_offs;
    uint8_t* pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_used[2] = {false, false};  // a DMA through the buffer has been queued: its event must be waited for before the buffer is written again
    hipStream_t copy_stream = nullptr;  // second stream: the remapped maps travel back while the rest of the pipeline runs
    size_t hcap_n = 0, hcap_wh = 0;
    int hcap_max_lines = 0;
    bool hcap_lineim = false;
    // tables
    DevBuf<double> d_taps, d_lgamma, d_ptab;
    DevBuf<int> d_centres;
    bool cost_history = false;          // lsd_set_cost_history: the region stage takes the images in the order of their cost in the last launch
    int hist_n = 0;                     // images of the launch whose counter records are in `stats` (0: none)
    lsd_params tab_params{};
    bool tab_valid = false;
    int tapR = 0;
    // createMapCache workspace
    DevBuf<unsigned long long> mc_claim;
    DevBuf<uint32_t> mc_fa, mc_fb;
    DevBuf<int> mc_ctl;                                 // spread flood: frontier sizes + per-chunk counts
    DevBuf<uint8_t> mc_in;
    DevBuf<double> mc_out;
    DevBuf<uint8_t> oc_in, oc_out;                      // occupancy-grid staging of the host entry point
    // staging of the host entry points of scan-to-map matching, FeatureScan and FeatureAssociation (one arena: each of them ends in a
    // stream synchronisation, so no two are live at once), and the per-sequence workspace of the device FeatureAssociation (k_fa.hip)
    DevBuf<uint8_t> stage;
    DevBuf<uint8_t> fa_buf;
    DevBuf<uint8_t> gm_mr_ws;                           // lsd_enqueue_grid_match_mr_device: U, the coarse slots, the counts and the pick's slots
    DevBuf<uint32_t> gr_volume;                         // lsd_enqueue_grid_response_device: the volume of R where the caller gives none
    DevBuf<uint8_t> gl_ws;                              // lsd_enqueue_grid_locate_device: the regions grid_locate_ws names
    DevBuf<uint8_t> gm_slots;                           // lsd_enqueue_grid_match_device: the per-(scan, angle) slots between its two kernels
    std::vector<int> fa_nf;                             // the host copy of the last localize enqueue's frame counts (its upload's source)
    // the fleet entries' map tables: the host copies their uploads read (as fa_nf) and the device records the kernels read; the first
    // LSD_MAX_MAPS of each belong to FeatureScan's entry, the rest to the two loops, so neither call disturbs the other's
    std::vector<lsd_map_ref> map_tab_host = std::vector<lsd_map_ref>(2 * LSD_MAX_MAPS);
    DevBuf<lsd_map_ref> map_tab;
    int fa_lds_bound = kFaLdsMax;                       // kept candidates sorted in LDS up to this many (kTunings "FA_LDS")
    // lsd_gather_lines: this rank's padded counts + offsets, and its slab of packed line records
    DevBuf<int32_t> ga_cnt;
    DevBuf<lsd_line> ga_slab;
    hipEvent_t ga_ev = nullptr;         // recorded behind the collectives of the last lsd_gather_lines (they read ga_cnt / ga_slab)
    bool ga_ev_valid = false;
    // options
    int stop_after = 0;
    int tun_groups = -1;                // the 8-wave region stage as persistent workgroups (k_region.hip: k_region): -1 = as many as CUs when the batch has more images than that, 0 = never
    DevBuf<int> pcount;                 // ... and the launch's image counter
    bool trace = false;
    bool fused_front = true;            // lsd_set_fused_front: K1 + K2 as one kernel where it applies (use_front)
    bool fused_lines = true;            // lsd_set_fused_lines: K5 by the region stage's workgroups, image by image, where it applies
    bool last_lines_fused = false;      // the last launch wrote its lines in the region stage: "lines" of lsd_last_timings reads exactly 0
    int scan_cap = kRdpShortMaxLen;     // lsd_set_scan_capacity: readings per scan (the stride) FeatureScan and the ingest entries take
    bool rdp_long_ready = false;        // the long FeatureScan kernels' dynamic-LDS limit covers scan_cap (prepare_rdp_long)
    int host_max_lines = 8192;
    // last run
    Geom geom{};
    int last_n = 0;
    int last_max_lines = 0;
    int32_t* last_counts = nullptr;
    // the last call took the fused front end: no Gaussian image exists, LSD_DBG_GAUSS recomputes the requested one from the call's input
    // (last_in; last_remapped: that input has been rewritten in place since, LSD_FLAG_WRITEBACK_MAP) into dbg_gauss
    bool last_fused = false, last_remapped = false;
    const uint8_t* last_in = nullptr;
    DevBuf<double> dbg_gauss;
    hipEvent_t ev[7]{};
    bool ev_valid = false;
    hipEvent_t ev_done = nullptr;      // end of the last enqueue: a later enqueue on ANOTHER stream waits for it (shared workspace)
    bool done_valid = false;
    hipStream_t done_stream = nullptr; // the stream ev_done was recorded on (last_stream moves with every entry point, this one with the detector only)
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return e_ == hipErrorOutOfMemory ? LSD_ERR_NOMEM : LSD_ERR_HIP;                       \
        }                                                                                         \
    } while (0)

// What an enqueue entry does once it has accepted its arguments: on the context's device, `launch(s)` readies its workspace, if it has
// any, and enqueues on the caller's stream s.  It returns a status (HIPCHK works inside it); a launch the runtime refused is an error too.
template <class Launch>
int enqueue_on(lsd_ctx* c, void* stream, Launch&& launch) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int st = launch(s);
    if (st != LSD_OK) return st;
    HIPCHK(c, hipGetLastError());
    c->last_stream = s;
    return LSD_OK;
}

// One pass over the staged regions of a host convenience (stage_round_trip below): each region is named once -- its device pointer, the
// host array it mirrors, the element count -- by the way it travels: in, out, both, or scratch, which only the device uses.
class StagePass {
public:
    enum What { kCarve = 0, kUp = 1, kDown = 2 };
    StagePass(What what, Carver* carver, hipStream_t s) : what_(what), carver_(carver), s_(s) {}
    template <class T> void in(T*& d, const T* h, size_t n) { region(d, const_cast<T*>(h), n, kUp); }
    template <class T> void out(T*& d, T* h, size_t n) { region(d, h, n, kDown); }
    template <class T> void both(T*& d, T* h, size_t n) { region(d, h, n, kUp | kDown); }
    template <class T> void scratch(T*& d, size_t n) { region(d, static_cast<T*>(nullptr), n, 0); }
    hipError_t status = hipSuccess;   // of the pass's copies: nothing is queued behind one that failed

private:
    template <class T> void region(T*& d, T* h, size_t n, int travels) {
        if (what_ == kCarve) (*carver_)(d, n);
        else if ((travels & what_) && h && n && status == hipSuccess)
            status = what_ == kUp ? hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s_)
                                  : hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, s_);
    }
    What what_;
    Carver* carver_;
    hipStream_t s_;
};

// What a host convenience does once it has accepted its arguments: one round trip through c->stage.  `plan(k)` names the regions
// (StagePass); they are carved in that order (lsd_devbuf.h: carve), the uploads queued on c->stream, `body()` run -- the device entry on
// the staged pointers and whatever else the convenience queues with it, on c->stream -- the downloads queued behind it and the stream
// drained.  A region whose host pointer is null or whose count is 0 is carved and not copied.  From the first upload on nothing returns
// before the stream is drained, whether HIP failed or the body refused: the uploads still read the caller's arrays.
template <class Plan, class Body>
int stage_round_trip(lsd_ctx* c, Plan&& plan, Body&& body) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, carve(c->stage, [&](Carver& k) { StagePass place(StagePass::kCarve, &k, nullptr); plan(place); }));
    StagePass up(StagePass::kUp, nullptr, c->stream), down(StagePass::kDown, nullptr, c->stream);
    plan(up);
    const int st = up.status == hipSuccess ? body() : LSD_OK;
    if (up.status == hipSuccess && st == LSD_OK) plan(down);
    const hipError_t drained = hipStreamSynchronize(c->stream);
    HIPCHK(c, up.status);
    if (st != LSD_OK) return st;
    HIPCHK(c, down.status);
    HIPCHK(c, drained);
    return LSD_OK;
}
