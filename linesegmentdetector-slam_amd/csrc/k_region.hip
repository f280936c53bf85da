// k_region.hip -- K4: the region stage (seed loop) of LSD, one workgroup of NW wavefronts per image (gfx950).
//
// Replaces the seed loop of myLineSegmentDetector (LSD/myLSD.cpp:219-272) and its callees
// RegionGrower (:491-590), CenterGetter/OrientationGetter/RectangleConverter (:592-734),
// RegionRadiusReducer (:736-802), Refiner (:804-880), LogGammaCalculator (:882-924),
// RectangleNFACalculator (:926-1059) and RectangleImprover (:1061-1158).
//
// The reference is strictly sequential: seeds are visited in sorted order and each one sees the
// usedMap left by all earlier ones.  What actually couples two seeds is small, though: a seed's whole
// evaluation (grow, rectangle, refine, NFA) reads usedMap only through "is this pixel banned
// (== 1)?", and only ACCEPTED lines ever set a pixel to 1 (rejected regions set 2, which stays
// growable; small/failed regions set nothing).  So the wavefronts of a workgroup evaluate seeds
// SPECULATIVELY ahead of a commit cursor and commit in seed order:
//   * seeds are handed out in chunks of 32; every seed has a record in an LDS ring (state byte, snapshot epoch, a result word);
//   * a wavefront first CLASSIFIES the seeds of its chunk, eight at a time: its eight 8-lane groups each grow one seed's region
//     out of a window of 16 x kWinRows pixels in LDS.  Nine regions in ten stay below regThre pixels and end there (nothing to mark, :228);
//   * the others wait for a FULL evaluation by whichever wave is free: grow() with all 64 lanes (8 frontier pixels x 8
//     neighbours per batch out of an LDS tile cache of packed pixel words), rectangle, Refiner incl. its regrow, NFA
//     (eval_seed()); results that mark nothing are published in the ring, results that mark usedMap are stashed (record +
//     pixel list in one of the wave's result slots in HBM) and committed when the cursor reaches them;
//   * at its turn a result is valid if its seed is still unused and no MEMBER of its grown lists was banned since its
//     snapshot -- accepted pixels carry their line's epoch (epochmap), per-tile accept epochs and the boxes of recently
//     accepted lines are the first filters; an invalid result is evaluated again at the cursor, where everything earlier is
//     committed;
//   * commit = mark usedMap (code 3 + epoch, or 2), append the rectangle, advance the cursor (up to 64 records per step);
//   * how far ahead the waves work adapts (deeper while waves idle, shallower after a redo);
//   * a workgroup whose image is done lends its wavefronts to images that are still busy evaluating ("Help from other
//     workgroups" in the kernel): requests and answers through HBM, the owner's cursor commits.
// The committed sequence of decisions is therefore exactly the sequential one (DESIGN.md section 4 has the
// measurements behind every choice, DESIGN_NOTES.md the variants that were tried and dropped).
// Inside a wavefront the lanes cooperate where the order of evaluation can be kept:
//   * region growing: candidates are classified against the ESTIMATED sum vector of the region with a rigorous
//     margin, the exact fp64 angle sums (reference order = list order) are caught up lazily from the list;
//   * rectangle moments: products per lane, SERIAL accumulation in list order (bit-exact sums);
//   * NFA pixel count: the rectangle's columns are flattened with a wave prefix sum and counted
//     with ballot/popcount;
//   * usedMap marking: only the region's pixels are visited (the reference scans the whole image).
// The stages are private headers under region/, each included once below, inside the variant namespace, in this order (each uses the ones before it):
//   config.h  build configuration (LSD_REGION_* defaults), sizes, set labels, Rec / WState / RCtx
//   stats.h   counters (ST_*, STAT ...) and the near-tie accounting (kTie*, TIES_AT)
//   lds.h     the namespace-scope LDS: per-wave arena and its views, the g_* objects, EvalOut, stage4 / acc32
//   wave.h    wave primitives: ballots, L2 accesses and fences, uni / uglobal, DPP reductions, lget / lset
//   tiles.h   the LDS tile cache and the member masks in HBM
//   grow.h    exact_sums, grow() / grow_any() (RegionGrower, by tolerance class)
//   rect.h    rect_convert, rec_density, radius_reduce (RegionRadiusReducer)
//   nfa.h     log_gamma_dev, nfa_count, nfa_tail, improve (RectangleImprover)
//   eval.h    refine_tol (Refiner), mark_region, list_bbox, certify_set, eval_seed
// This file keeps the commit ring, region_image (the scheduler), the kernel and the two launchers.
#include "lsd_internal.h"
#include "devmath.h"
#include "lines_dev.h"

// The file is compiled twice (Makefile): LSD_REGION_NW = 4 (two images per CU: the batch path, all 512 workgroups of the
// bench batch resident at once) and LSD_REGION_NW = 8 (one image per CU, 8 speculative wavefronts per image: lower
// latency per image, chosen when the batch leaves CUs idle anyway).  Everything lives in a per-variant namespace.
#ifndef LSD_REGION_NW
#define LSD_REGION_NW 4
#endif
#if LSD_REGION_NW == 8
#define RVAR w8
#else
#define RVAR w4
#endif

namespace lsdhip {
namespace RVAR {
#include "region/config.h"
#include "region/stats.h"
#include "region/lds.h"
#include "region/wave.h"
#include "region/tiles.h"
#include "region/grow.h"
#include "region/rect.h"
#include "region/nfa.h"
#include "region/eval.h"

// (developer build only: the seed loop can be cut short for the cost-probe experiments of DESIGN_NOTES.md; the product runs them all)
#ifdef LSD_REGION_STATS
__device__ __forceinline__ int seed_limit(int cnt, int stop) { return stop > 0 ? min(cnt, stop) : cnt; }
#else
__device__ __forceinline__ int seed_limit(int cnt, int) { return cnt; }
#endif
__device__ __forceinline__ int lds_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Commit ring: one record per seed in flight (index = seed number & (RW-1)).
//   R_EMPTY  reserved by a wave (part of its chunk of seeds), not classified yet
//   R_SKIP   the seed pixel was already used when it was looked at (monotone, so final): nothing to do
//   R_LIGHT  a small region (:228, nothing to mark) grown by the small-region grower: aux = box of what it examined,
//            relative to the seed; whoever advances the cursor checks that no line accepted since the snapshot touches it
//   R_LIGHTL a full evaluation without marks (small region :228 or refine failed :237): aux = result slot (box and list
//            sizes in the slot table, the lists in the slot); checked like R_LIGHT, by the pixels themselves if the box is hit
//   R_BIG    the small-region grower gave the seed up (its region reaches regThre pixels, leaves the seed's window, or a
//            test was too close to call): waits for a full evaluation by any wave
//   R_EVAL   being evaluated in full, ahead of the cursor
//   R_STASH  evaluated with a result that marks usedMap: record and pixel list wait in the owner's result slot (aux);
//            whoever moves the cursor over it validates and commits it
//   R_REDO   a speculative result was invalidated (or abandoned): must be evaluated again at the cursor
//   R_BUSY   being evaluated at the cursor
//   R_REMOTE given to the wavefronts of other workgroups that help with this image (aux = request number); R_XLIGHTL / R_XSTASH:
//            their answers, R_LIGHTL / R_STASH with the lists and the record in the HELPER's result slot (aux = request number,
//            the slot and the box in the request table)
//   R_SETL   the seed belongs to a live certified set (aux = its label): the evaluation is known without growing anything (no marks);
//            valid at the cursor iff the set is still alive
enum { R_EMPTY = 0, R_SKIP = 1, R_LIGHT = 2, R_REDO = 3, R_BUSY = 4, R_STASH = 5, R_BIG = 6, R_EVAL = 7, R_LIGHTL = 8,
       R_REMOTE = 9, R_XLIGHTL = 10, R_XSTASH = 11, R_SETL = 12 };
constexpr int kHelpIdle = 50;             // looks without a request after which a helper wavefront leaves an image
constexpr int RW = 256 * NW;              // records in flight: how far the hand-out may run ahead of the cursor
constexpr int CH = 32;                    // seeds a wave reserves at a time (its chunk)

struct Ring {
    alignas(4) uint8_t state[RW];
    uint16_t snap[RW];   // accept epoch (mod 2^16) the result was computed against
    uint32_t aux[RW];    // see above
};
struct SlotTab {         // per result slot (wave * NS + slot) of a full evaluation published as R_LIGHTL
    short box[NW * NS][4];
    uint32_t lcnt[NW * NS];   // n1 + 1 | n2 << 16 (n1 + 1 == 0: the lists were not kept, box check only)
};
__device__ __forceinline__ int st_ld(uint8_t* p) { return (int)__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_st(uint8_t* p, int v) { __hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
// compare-and-swap of ONE state byte (call it from one lane): the containing word is swapped, and the swap is retried as long
// as only the other three bytes of the word have changed in between
__device__ __forceinline__ bool st_cas(uint8_t* base, int idx, int expect, int desired) {
    uint32_t* const wp = reinterpret_cast<uint32_t*>(base) + (idx >> 2);
    const int sh = (idx & 3) * 8;
    while (true) {
        const uint32_t oldw = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (((oldw >> sh) & 0xffu) != (uint32_t)expect) return false;
        const uint32_t neww = (oldw & ~(0xffu << sh)) | ((uint32_t)desired << sh);
        if (atomicCAS(wp, oldw, neww) == oldw) return true;
    }
}

// minimum / maximum over the 8 lanes of a group for small non-negative integers (exact in fp32)
__device__ __forceinline__ int imin8(int v) { return (int)min8((float)v); }
__device__ __forceinline__ int imax8(int v) { return -(int)min8(-(float)v); }

// One image's region stage by the calling workgroup; `bid` is the workgroup's place in the launch's image order (blockIdx.x of the
// one-workgroup-per-image launch; the next number of the launch's counter for a persistent workgroup, see k_region below).
__device__ __forceinline__ void region_image(const Geom& g, const Buffers& b, uint32_t id_base, const int bid, const int nimg) {
    __shared__ int s_next, s_commit, s_epoch, s_lines, s_ntrace, s_nseeds, s_lock, s_nbig, s_depth, s_abort, s_nsets;
    __shared__ int s_scan[NW];                              // the waves' counts of potential seeds (the seed scan at the start)
    __shared__ short s_ring[RING][4];
    __shared__ Ring rg;
    __shared__ SlotTab stab;
    // seeds given to helpers: request j holds seed s_xk[j] (-1: free, -2: answered -- the answer, in the image's record of the
    // help protocol in HBM, waits for the cursor)
    __shared__ int s_nhelp, s_xout, s_xlock, s_xreg, s_xpub, s_idlecnt, s_xc_last, s_xt_last, s_workbound;
    __shared__ int s_xk[kXReq];

    // The last b.npool workgroups of the launch own no image: they are HELPERS from the start (the host adds them when the images
    // leave workgroup slots of the device free, see "Help from other workgroups" below), with a workspace slot of their own.
    const bool pool = bid >= nimg;
    const size_t img = pool ? (size_t)bid : (size_t)b.order[bid];                         // heaviest images first (k_order); pool: its workspace slot
    uint32_t* const xr = (b.xq && !pool) ? b.xq + img * (size_t)kXStride : nullptr;        // this image's record of the help protocol
    uint32_t* const xhdr = b.xq ? b.xq + (size_t)nimg * kXStride : nullptr;                 // ... and the launch's
    if (threadIdx.x == 0 && xhdr && !pool) atomicAdd(&xhdr[0], 1u);
    // when the launch's first workgroup started (s_memrealtime, 100 MHz, the same on every CU; low 32 bits | 1): what "running long"
    // is measured against (below)
    if (threadIdx.x == 0 && xhdr) atomicCAS(&xhdr[4], 0u, (uint32_t)__builtin_amdgcn_s_memrealtime() | 1u);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = g.w, h = g.h;
    const size_t npx = (size_t)g.npx;

    RCtx c;
    c.w = w; c.h = h; c.lane = lane; c.wave = wave;
    c.mag = b.mag + img * npx; c.deg = b.deg + img * npx; c.pw = b.pw + img * npx; c.epochmap = b.epochmap + img * npx;
    c.sets = (pool || !b.sets) ? nullptr : b.sets + img * (size_t)(kSetMax + 1);
    c.ltag = (id_base >> 20) & 0x3ffu;
    c.tep = b.tepoch + img * (size_t)(((w + 7) >> 3) * ((h + 7) >> 3));
    c.sc = b.sc + img * npx;
    c.tmask = b.stamps + (img * NW + wave) * (size_t)b.tm_stride;
    c.spill = b.spill + (img * NW + wave) * npx; c.gcopy = b.gcopy + (img * NW + wave) * npx;
    c.meta = b.wmeta + (img * NW + wave) * (size_t)b.mcap; c.mcap = b.mcap;
    c.tilesX = (w + 7) >> 3; c.id_base = id_base; c.id_budget = b.id_budget;
    if (lane == 0) {
        WState& ws = g_ws[wave];
        ws.cur_id = id_base; ws.gnum = 0; ws.has_copy = 0; ws.tm_pending = 0; ws.cache_epoch = -1; ws.members_cached = 0;
        ws.ex_upto = 0; ws.ex_sin = 0; ws.ex_cos = 0;
    }
    c.logNT = g.logNT; c.lgamma = b.lgamma; c.lg_count = b.lg_count; c.ptab = b.ptab;
    c.wslist = b.slist + (img * NW + wave) * (size_t)NS * b.gcap; c.gcap = b.gcap;
    if (threadIdx.x == 0) { g_par[0] = g.degThre; g_par[1] = g.regThre; g_par[2] = g.aliPro; g_par[3] = g.denThre; }
    if (lane == 0) g_ctx[wave] = c;                        // (c.lane is set by every reader)
    if (lane < kStatSlots) g_stat[c.wave][lane] = 0ull;
    const long long t_begin = (long long)__builtin_amdgcn_s_memtime();
    [[maybe_unused]] const long long rt_begin = (long long)__builtin_amdgcn_s_memrealtime();   // (100 MHz, the same on every CU)
    if (lane < NT) g_ttag[c.wave][lane] = -1;
    for (int j = threadIdx.x; j < RW / 4; j += 64 * NW) reinterpret_cast<uint32_t*>(rg.state)[j] = 0u;    // R_EMPTY
    if (threadIdx.x < kXReq) s_xk[threadIdx.x] = -1;
    if (c.sets) for (int j = threadIdx.x; j <= kSetMax; j += 64 * NW) st_l2(&c.sets[j], 0u);   // no certified set yet (labels of earlier launches carry another tag)
    if (!pool) {
        // this image's counter record and tile epochs start from zero (cleared here, not by fills in front of the launch: every dispatch
        // of a batch in flight waits for a hardware pipe; lsd_ctx.hip).  Nobody touches them before the barrier behind the seed scan below;
        // helpers of other workgroups only after this image has asked for them.
        if (b.stats) for (int j = threadIdx.x; j < kStatWords; j += 64 * NW) b.stats[img * kStatWords + j] = 0ll;
        const int ntile = c.tilesX * ((h + 7) >> 3);
        for (int j = threadIdx.x; j < ntile; j += 64 * NW) c.tep[j] = 0u;
    }

    const uint32_t* ord = b.ord + img * npx;
    uint32_t* seedidx = b.seedidx + img * npx;
    uint32_t* seedpos = b.seedpos + img * npx;
    const int nb = pool ? 0 : b.nb[img];
    double* recs = b.recs + img * (size_t)b.max_lines * 12;
    double* recs_scaled = b.recs_scaled + img * (size_t)b.max_lines * 4;
    SeedRec* trace = b.seeds ? reinterpret_cast<SeedRec*>(b.seeds) + img * npx : nullptr;
    int* rnum = b.rnum + img * (size_t)RW * 2;            // (num0, final_num << 2 | outcome) of published records: read by the seed trace only

    if (wave == NW - 1) {
        double st, ct;
        sincos_g(g.degThre < 1.5 ? g.degThre : 1.0, st, ct);
        if (lane == 0) { g_tol0[0] = g.degThre; g_tol0[1] = st; g_tol0[2] = ct; }
    }
    // ======== region_image 1/6: seed scan ========
    // potential seeds: sorted entries whose pixel is not below the gradient threshold (usedMap == 0 after K2), in sorted order.  Every
    // wave takes a contiguous share of the list, four chunks of 64 entries per trip to memory (an entry costs two dependent reads:
    // its position, then that pixel's word): first the counts, then -- the shares' offsets known -- the same walk again, writing
    // (one wave walking the whole list chunk by chunk took ~0.8 ms of a 2048 x 2048 map's 9).
    {
        const int nchunks = (nb + 63) >> 6, per = (nchunks + NW - 1) / NW;
        const int c0 = min(wave * per, nchunks), c1 = min(c0 + per, nchunks);
        const unsigned long long lt = (1ull << lane) - 1ull;
        int cnt = 0;
        for (int pass = 0; pass < 2; pass++) {
            for (int ch = c0; ch < c1; ch += 4) {
                uint32_t pq[4], cw[4];
                bool in[4];
                #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = (ch + u) * 64 + lane;
                    in[u] = ch + u < c1 && idx < nb;
                    pq[u] = ord[in[u] ? idx : 0];
                }
                #pragma unroll
                for (int u = 0; u < 4; u++) cw[u] = c.pw[pq[u]];
                #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool ok = in[u] && (cw[u] & 3u) == 0u;                   // :222
                    const unsigned long long m = ballot64(ok);
                    if (pass == 1 && ok) { const int o = cnt + __builtin_popcountll(m & lt); seedidx[o] = (uint32_t)((ch + u) * 64 + lane); seedpos[o] = pq[u]; }
                    cnt += __builtin_popcountll(m);
                }
            }
            if (pass == 0) {
                if (lane == 0) s_scan[wave] = cnt;
                __syncthreads();
                int off = 0, tot = 0;
                for (int v = 0; v < NW; v++) { const int t = s_scan[v]; off += v < wave ? t : 0; tot += t; }
                cnt = off;
                if (wave == 0 && lane == 0) { s_next = 0; s_commit = 0; s_epoch = 0; s_lines = 0; s_ntrace = 0; s_nseeds = seed_limit(tot, b.tun_stop); s_lock = 0; s_nbig = 0; s_depth = min(max(b.tun_soft, 2 * CH), RW - 128); s_abort = 0; s_nsets = 0; s_nhelp = 0; s_xout = 0; s_xlock = 0; s_xreg = 0; s_xpub = 0; s_idlecnt = 0; s_xc_last = 0; s_xt_last = (int)__builtin_amdgcn_s_memtime(); s_workbound = 0; }
            }
        }
        wg_fence();
        __syncthreads();
        if (xr) {                                           // helpers on other XCDs read seedpos[] as soon as a request names a seed
            if (wave == 0) agent_release();
            __syncthreads();
        }
    }
    const int nseeds = s_nseeds;

    // ======== region_image 2/6: cursor helpers (validity tests, trace, requeue_ahead, commit_marks) ========
    // How far the hand-out and the full evaluations may run ahead of the cursor (s_depth, in seeds).  The further ahead a region is
    // evaluated, the likelier a line accepted before its turn makes the work void (typical maps: many lines, short evaluations);
    // but where single evaluations take a millisecond (long sparse structures grown again and again without ever marking
    // anything) a short look-ahead leaves the other waves without work.  So the depth adapts: it grows while waves find nothing
    // to do within it, and shrinks when a speculative result is redone or discarded at the cursor.  Ring slots are reused no
    // sooner than 128 commits later.
    const int depth_min = min(max(b.tun_soft, 2 * CH), RW - 128), depth_max = min(max(b.tun_claim, depth_min), RW - 128);
    const int kDepthUp = b.tun_up, kDepthDown = b.tun_down;   // steps of the adaptive look-ahead
    const int kFeed = min(max(b.tun_feed, 1), 8);           // idle groups that make a wave fetch the windows of its next seeds (a memory round trip)
    // box overlap of record-style boxes against the lines accepted in epochs [snap, now)
    auto hit_since = [&](int snap, int now, int x0, int y0, int x1, int y1) -> bool {
        if (now - snap > RING) return true;
        bool hit = false;
        for (int ep = snap; ep < now; ep++) {
            const short* r = s_ring[ep & (RING - 1)];
            if (!(r[2] < x0 || r[0] > x1 || r[3] < y0 || r[1] > y1)) hit = true;
        }
        return hit;
    };
    auto write_trace = [&](int k, int num0, int fnum, int outcome, double logNFA) {
        if (lane == 0) {
            if (trace) {
                const int oidx = (int)seedidx[k];
                const uint32_t pp = seedpos[k];
                SeedRec tr;
                tr.order_idx = oidx; tr.x = (int)(pp % (uint32_t)w); tr.y = (int)(pp / (uint32_t)w);
                tr.num = num0; tr.outcome = outcome; tr.final_num = fnum; tr.logNFA = logNFA;
                trace[s_ntrace] = tr;
            }
            s_ntrace = s_ntrace + 1;
        }
    };
    // True if a MEMBER of a region's grown lists was banned by a line accepted in epoch >= snap: only then can the region's
    // evaluation differ from what it would be now.  (It read usedMap only as "banned?" of candidate pixels, :537.  A pixel it
    // examined and did NOT take -- the angle test failed every time it came up -- is skipped now instead of failing: the same
    // sequence of accepts, the same sums, the same lists.  A pixel it took would now be skipped: a different region.  So the
    // neighbours of the lists do not matter, the lists do.)  Accepted pixels carry their line's epoch + 1 in epochmap.
    auto examined_hit = [&](const uint32_t* lp, int cnt, int snap) -> bool {
        // first by tiles (tep[] is a few KB and stays in the cache): no line accepted since the snapshot has a pixel in any tile
        // a member lies in
        const int tX = c.tilesX;
        bool thit = false;
        for (int base = 0; base < cnt; base += 64) {
            const int k2 = base + lane;
            if (k2 < cnt) {
                const uint32_t pkx = lp[k2];
                const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
                if ((int)ld_l2(&c.tep[(y >> 3) * tX + (x >> 3)]) > snap) thit = true;
            }
        }
        if (!ballot64(thit)) return false;
        bool hit = false;
        for (int base = 0; base < cnt; base += 64) {
            const int k2 = base + lane;
            if (k2 < cnt) {
                const uint32_t pkx = lp[k2];
                const size_t q = (size_t)(pkx >> 16) * w + (pkx & 0xffffu);
                if ((c.pw[q] & 3u) == kPwLine && (int)c.epochmap[q] > snap) hit = true;
            }
        }
        return ballot64(hit) != 0ull;
    };
    // the same question for a box: true if a tile overlapping it holds a pixel of a line accepted in epoch >= snap
    auto box_tile_hit = [&](int snap, int x0, int y0, int x1, int y1) -> bool {
        const int tX = c.tilesX;
        const int xa = max(x0, 0) >> 3, xb = min(x1, w - 1) >> 3, ya = max(y0, 0) >> 3, yb = min(y1, h - 1) >> 3;
        bool hit = false;
        for (int ty = ya; ty <= yb; ty++)
            for (int tx = xa; tx <= xb; tx++)
                if ((int)ld_l2(&c.tep[ty * tX + tx]) > snap) hit = true;
        return hit;
    };
    // Commits a result that marks usedMap (accepted line: code 3 + epoch; rejected region: code 2), at the cursor, under
    // the cursor lock: pv = lane j < 12: field j of the rectangle (structRec order); m_src: the pixels to mark (null: this
    // wave's own last grow).
    // A line has just been accepted (seed k, box mb).  A finished result further ahead that it invalidates would be found
    // invalid when the cursor reaches it and evaluated again THERE, with every other wave waiting (images with many lines on
    // the same structures spent 45 % of their time in such evaluations).  Found now, it goes back to the seeds that wait for a
    // full evaluation and is redone by whichever wave is free while the cursor works its way towards it.  (Called by the wave
    // that owns the cursor; nobody else touches a finished record.)
    auto requeue_ahead = [&](int k, const Box& mb) {
        const int lim = min(lds_ld(&s_next), nseeds);
        const int now = lds_ld(&s_epoch);
        for (int base = k + 1; base < lim; base += 64) {
            const int idx = base + lane;
            const int rr = idx & (RW - 1);
            const int stl = idx < lim ? st_ld(&rg.state[rr]) : R_EMPTY;
            int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
            if (stl == R_LIGHT) {
                const uint32_t ax = rg.aux[rr], sp = seedpos[idx];
                const int sxp = (int)(sp % (uint32_t)w), syp = (int)(sp / (uint32_t)w);
                x0 = sxp + (int)(ax & 63u) - 32; y0 = syp + (int)((ax >> 6) & 63u) - 32;
                x1 = sxp + (int)((ax >> 12) & 63u) - 32; y1 = syp + (int)((ax >> 18) & 63u) - 32;
            } else if (stl == R_LIGHTL) {
                const uint32_t ax = rg.aux[rr];
                x0 = stab.box[ax][0]; y0 = stab.box[ax][1]; x1 = stab.box[ax][2]; y1 = stab.box[ax][3];
            } else if (stl == R_STASH) {
                const double* P = b.pend + (img * (size_t)(NW * NS) + rg.aux[rr]) * 24;
                x0 = (int)P[18]; y0 = (int)P[19]; x1 = (int)P[20]; y1 = (int)P[21];
            }
            if (stl == R_SETL && ld_l2(&c.sets[rg.aux[rr]]) == 0u) {           // its set ended (with this line, or earlier): a full evaluation then
                st_st(&rg.state[rr], R_BIG); atomicAdd(&s_nbig, 1);
                DSTAT(ST_DEPTHUP, 1);
            }
            unsigned long long hm = ballot64(!(mb.x1 < x0 || mb.x0 > x1 || mb.y1 < y0 || mb.y0 > y1) && x1 >= x0);
            while (hm) {
                const int l = __builtin_ctzll(hm);
                hm &= hm - 1ull;
                const int st1 = __builtin_amdgcn_readlane(stl, l), r1 = (base + l) & (RW - 1);
                const uint32_t ax1 = rg.aux[r1];
                const int snap = now - ((now - (int)rg.snap[r1]) & 0xffff);
                bool conflict = true;
                if (st1 == R_LIGHT) {
                    conflict = box_tile_hit(snap, __builtin_amdgcn_readlane(x0, l), __builtin_amdgcn_readlane(y0, l), __builtin_amdgcn_readlane(x1, l), __builtin_amdgcn_readlane(y1, l));
                } else {
                    const size_t gs = img * (size_t)(NW * NS) + ax1;
                    int n = -1;
                    if (st1 == R_LIGHTL) { const uint32_t lc = stab.lcnt[ax1]; if (lc & 0xffffu) n = (int)(lc & 0xffffu) - 1 + (int)(lc >> 16); }
                    else { const long long pk3 = (long long)b.pend[gs * 24 + 22]; const int n1 = (int)(pk3 % 32768ll) - 1; if (n1 >= 0) n = n1 + (int)((pk3 / 32768ll) % 32768ll); }
                    if (n >= 0) conflict = examined_hit(b.slist + gs * b.gcap, n, snap);
                }
                if (conflict) {
                    if (lane == 0) { st_st(&rg.state[r1], R_BIG); atomicAdd(&s_nbig, 1); }
                    DSTAT(ST_DEPTHUP, 1);
                }
            }
        }
    };
    auto commit_marks = [&](int k, int num0, int fnum, int outcome, double logNFA, double pv, const uint32_t* m_src, int m_cnt) {
        write_trace(k, num0, fnum, outcome, logNFA);
        if (outcome == 2) {                                                          // :242-250
            (void)mark_region(c.wave, 0u, m_src, m_cnt);
        } else if (outcome == 3) {
            const int li = s_lines;
            if (li < b.max_lines) {
                if (lane < 12) recs[(size_t)li * 12 + lane] = pv;                    // structRec as accepted
                if (lane < 4) recs_scaled[(size_t)li * 4 + lane] = g.sca != 1 ? (pv - 1.0) / g.sca + 1 : pv;   // x1 y1 x2 y2, :252-258
            }
            const Box mb = mark_region(c.wave, (uint32_t)(lds_ld(&s_epoch) + 1), m_src, m_cnt);   // :259-265 (+ the line's epoch)
            wg_fence();                                   // the marks must be visible before the epoch moves
            if (xr) agent_release();                      // ... to the helpers on other CUs as well
            if (lane == 0) {
                const int ep = s_epoch;
                short* r = s_ring[ep & (RING - 1)];
                r[0] = (short)mb.x0; r[1] = (short)mb.y0; r[2] = (short)mb.x1; r[3] = (short)mb.y1;
                s_lines = li + 1;
                lds_st(&s_epoch, ep + 1);
                if (xr) st_l2(&xr[0], (uint32_t)(ep + 1));
            }
            invalidate_tiles(c);                          // this wave's cached ban flags are stale now
            g_ws[wave].cache_epoch = -1;
            wg_fence();
            if (b.tun_requeue) requeue_ahead(k, mb);
        }
        wg_fence();                                       // marks + ring visible before the cursor moves
    };
    // ======== region_image 3/6: advance() -- the commit cursor ========
    // Moves the commit cursor over finished records (one wave at a time, whichever comes by): skipped seeds, results
    // without marks (after checking that they are still valid), and STASHED results of ANY wave -- everything a commit
    // needs sits in the owner's result slot in HBM, so the cursor never waits for an owner that is busy with a long
    // speculative evaluation further ahead.
    auto advance = [&]() {
        int got = 0;
        if (lane == 0) got = atomicCAS(&s_lock, 0, 1) == 0 ? 1 : 0;
        got = __builtin_amdgcn_readfirstlane(got);
        if (!got) return;
        while (true) {
            int f = lds_ld(&s_commit);
            if (f >= nseeds) break;
            if (!trace) {
                // a run of up to 64 records that need nothing but the cursor's nod (skipped seeds, results without marks that no
                // line accepted since their snapshot can have touched), one record per lane
                const int now = lds_ld(&s_epoch);
                const int idx = f + lane;
                const int rr = idx & (RW - 1);
                const int stl = idx < nseeds ? st_ld(&rg.state[rr]) : R_EMPTY;
                const uint32_t sp = idx < nseeds ? seedpos[idx] : 0u;           // (used only when a box has to be placed)
                bool ok = stl == R_SKIP;
                if (stl == R_SETL) ok = ld_l2(&c.sets[rg.aux[rr]]) != 0u;          // (alive: no member of the set was ever banned)
                if (stl == R_LIGHT || stl == R_LIGHTL) {
                    const int d = (now - (int)rg.snap[rr]) & 0xffff;
                    ok = d == 0;
                    if (!ok) {
                        const uint32_t ax = rg.aux[rr];
                        int x0, y0, x1, y1;
                        if (stl == R_LIGHT) {
                            const int sxp = (int)(sp % (uint32_t)w), syp = (int)(sp / (uint32_t)w);
                            x0 = sxp + (int)(ax & 63u) - 32; y0 = syp + (int)((ax >> 6) & 63u) - 32;
                            x1 = sxp + (int)((ax >> 12) & 63u) - 32; y1 = syp + (int)((ax >> 18) & 63u) - 32;
                        } else { x0 = stab.box[ax][0]; y0 = stab.box[ax][1]; x1 = stab.box[ax][2]; y1 = stab.box[ax][3]; }
                        // (the tile test only for the small boxes: a full evaluation's box may span the image, its lists say more)
                        ok = !hit_since(now - d, now, x0, y0, x1, y1) || (stl == R_LIGHT && !box_tile_hit(now - d, x0, y0, x1, y1));
                    }
                }
                const unsigned long long okm = ballot64(ok);
                const int run = okm == ~0ull ? 64 : __builtin_ctzll(~okm);
                if (run > 0) {
                    const unsigned long long runm = run == 64 ? ~0ull : (1ull << run) - 1ull;
                    const int nl = __builtin_popcountll(ballot64(stl != R_SKIP) & runm);
                    if (lane < run) rg.state[rr] = (uint8_t)R_EMPTY;
                    if (lane == 0) { s_ntrace = s_ntrace + nl; lds_st(&s_commit, f + run); }
                    f += run;
                    if (run == 64 || f >= nseeds) continue;
                }
            }
            const int r = f & (RW - 1);
            const int st = st_ld(&rg.state[r]);
            if (st == R_SKIP) {
                if (lane == 0) { rg.state[r] = (uint8_t)R_EMPTY; lds_st(&s_commit, f + 1); }
                continue;
            }
            if (st == R_LIGHT || st == R_LIGHTL || st == R_XLIGHTL) {
                const int now = lds_ld(&s_epoch);
                const int d = (now - (int)rg.snap[r]) & 0xffff, snap = now - d;
                const uint32_t ax = rg.aux[r];
                if (d != 0) {
                    int x0, y0, x1, y1;
                    if (st == R_LIGHT) {
                        const uint32_t sp = seedpos[f];
                        const int sxp = (int)(sp % (uint32_t)w), syp = (int)(sp / (uint32_t)w);
                        x0 = sxp + (int)(ax & 63u) - 32; y0 = syp + (int)((ax >> 6) & 63u) - 32;
                        x1 = sxp + (int)((ax >> 12) & 63u) - 32; y1 = syp + (int)((ax >> 18) & 63u) - 32;
                    } else if (st == R_LIGHTL) { x0 = stab.box[ax][0]; y0 = stab.box[ax][1]; x1 = stab.box[ax][2]; y1 = stab.box[ax][3]; }
                    else {
                        const uint32_t b0 = ld_l2(&xr[3 * kXReq + ax * 8 + 3]), b1 = ld_l2(&xr[3 * kXReq + ax * 8 + 4]);
                        x0 = (int)(b0 & 0xffffu); y0 = (int)(b0 >> 16); x1 = (int)(b1 & 0xffffu); y1 = (int)(b1 >> 16);
                    }
                    if (hit_since(snap, now, x0, y0, x1, y1) && (st != R_LIGHT || box_tile_hit(snap, x0, y0, x1, y1))) {
                        bool conflict = true;
                        const uint32_t lc = st == R_LIGHTL ? stab.lcnt[ax] : st == R_XLIGHTL ? ld_l2(&xr[3 * kXReq + ax * 8 + 5]) : 0u;
                        if ((lc & 0xffffu) != 0u) {   // the lists are still in their slot: look at the pixels themselves
                            const size_t gs = st == R_LIGHTL ? img * (size_t)(NW * NS) + ax : (size_t)ld_l2(&xr[3 * kXReq + ax * 8 + 1]);
                            wg_fence();
                            conflict = examined_hit(b.slist + gs * b.gcap, (int)(lc & 0xffffu) - 1 + (int)(lc >> 16), snap);
                        }
                        if (conflict) {
                            STAT(ST_REDO, 1);
                            if (lane == 0) {
                                if (st == R_XLIGHTL) s_xk[ax] = -1;
                                st_st(&rg.state[r], R_REDO); lds_st(&s_depth, max(depth_min, lds_ld(&s_depth) - kDepthDown));
                            }
                            break;
                        }
                    }
                }
                if (st == R_XLIGHTL && lane == 0) s_xk[ax] = -1;
                bool used_now = false;
                if (trace) used_now = (c.pw[seedpos[f]] & 3u) != 0u;          // the reference skips it then (:222): no record
                if (trace && !used_now) {
                    const int no = rnum[r * 2 + 1];
                    write_trace(f, rnum[r * 2], no >> 2, no & 3, 0.0);
                } else if (!trace) write_trace(f, 0, 0, 0, 0.0);
                if (lane == 0) { rg.state[r] = (uint8_t)R_EMPTY; lds_st(&s_commit, f + 1); }
                continue;
            }
            if (st == R_SETL) {
                if (ld_l2(&c.sets[rg.aux[r]]) == 0u) {                             // the set ended before the seed's turn: evaluate in full, here
                    STAT(ST_REDO, 1);
                    if (lane == 0) { st_st(&rg.state[r], R_REDO); lds_st(&s_depth, max(depth_min, lds_ld(&s_depth) - kDepthDown)); }
                    break;
                }
                bool used_now = false;
                if (trace) used_now = (c.pw[seedpos[f]] & 3u) != 0u;               // the reference skips it then (:222): no record
                if (trace && !used_now) {
                    const int no = rnum[r * 2 + 1];
                    write_trace(f, rnum[r * 2], no >> 2, no & 3, 0.0);
                } else if (!trace) write_trace(f, 0, 0, 0, 0.0);
                if (lane == 0) { rg.state[r] = (uint8_t)R_EMPTY; lds_st(&s_commit, f + 1); }
                continue;
            }
            if (st == R_STASH || st == R_XSTASH) {
                // ---- a stashed result at the cursor: is it still what the sequential run would get? ----
                const uint32_t ax = rg.aux[r];
                const size_t lr = st == R_STASH ? img * (size_t)(NW * NS) + ax : (size_t)ld_l2(&xr[3 * kXReq + ax * 8 + 1]);   // the result slot, of this image's waves or of a helper's
                wg_fence();
                if (st == R_XSTASH && lane == 0) s_xk[ax] = -1;                   // (whatever happens below, the request is over)
                const double pv = b.pend[lr * 24 + (lane < 24 ? lane : 0)];
                const double logNFA = rl(pv, 12);
                const int outcome = (int)rl(pv, 14), num0 = (int)rl(pv, 15), num = (int)rl(pv, 16), m_cnt = (int)rl(pv, 17);
                const int x0 = (int)rl(pv, 18), y0 = (int)rl(pv, 19), x1 = (int)rl(pv, 20), y1 = (int)rl(pv, 21);
                const int snap = (int)rl(pv, 23);
                const long long pk3 = (long long)rl(pv, 22);
                const int st_n1 = (int)(pk3 % 32768ll) - 1, st_n2 = (int)((pk3 / 32768ll) % 32768ll);
                const uint32_t* st_list = b.slist + lr * b.gcap;
                const uint32_t* m_src = st_list + (int)(pk3 / (32768ll * 32768ll));
                if ((c.pw[seedpos[f]] & 3u) != 0u) {       // an earlier seed marked the pixel meanwhile: the reference skips it (:222)
                    STAT(ST_DISCARD, 1);
                    if (lane == 0) { rg.state[r] = (uint8_t)R_EMPTY; lds_st(&s_commit, f + 1); lds_st(&s_depth, max(depth_min, lds_ld(&s_depth) - kDepthDown)); }
                    continue;
                }
                const int now = lds_ld(&s_epoch);
                if (now != snap && hit_since(snap, now, x0, y0, x1, y1)) {
                    bool conflict = true;
                    if (st_n1 >= 0) conflict = examined_hit(st_list, st_n1 + st_n2, snap);   // the pixels themselves
                    if (conflict) {
                        STAT(ST_REDO, 1);
                        if (lane == 0) { st_st(&rg.state[r], R_REDO); lds_st(&s_depth, max(depth_min, lds_ld(&s_depth) - kDepthDown)); }     // evaluate again; everything earlier is committed now
                        break;
                    }
                }
                commit_marks(f, num0, num, outcome, logNFA, pv, m_src, m_cnt);
                if (lane == 0) { rg.state[r] = (uint8_t)R_EMPTY; lds_st(&s_commit, f + 1); }
                continue;
            }
            break;
        }
        if (xr && lane == 0) st_l2(&xr[1], (uint32_t)lds_ld(&s_commit));     // (helpers free their result slots behind the cursor)
        if (lane == 0) lds_st(&s_lock, 0);
    };

    // ======== region_image 4/6: help protocol, the owner's side (xpoll, xservice, xexport) ========
    // ---- Help from other workgroups ----
    // The batch ends with its heaviest images: long sparse structures regrown from hundreds of seeds, millisecond evaluations that
    // are independent of one another, on one CU each while the CUs that have finished their images idle.  So a workgroup whose
    // image is done -- once every workgroup of the launch has started -- turns its wavefronts into HELPERS (the loop below, second
    // half): each attaches itself to an image that has asked for help, takes seeds that wait for a full evaluation from that
    // image's request table in HBM, evaluates them speculatively against that image's arrays with its own workspace, and answers
    // with what a local evaluation publishes: lists and record in the helper's own result slot, the rest in an 8-word message.
    // The owner's cursor validates and commits such an answer exactly like a local result, so nothing of the order of decisions
    // changes.  What crosses CUs goes through L2 (agent-scope atomics) behind release / acquire fences: bans and their epoch from
    // the owner to the helper, lists and records back.  A request nobody has taken when the cursor reaches it is taken back.
    auto xlock = [&]() -> bool {
        int got = 0;
        if (lane == 0) got = atomicCAS(&s_xlock, 0, 1) == 0 ? 1 : 0;
        return __builtin_amdgcn_readfirstlane(got) != 0;
    };
    auto xunlock = [&]() { wg_fence(); if (lane == 0) lds_st(&s_xlock, 0); };
    // takes the answers that have arrived into the ring; learns how many helpers the image has and tells them its backlog
    auto xpoll = [&]() -> bool {
        if (!xlock()) return false;
        const int kx = lane < kXReq ? s_xk[lane] : -1;
        const uint32_t fl = kx >= 0 ? ld_l2(&xr[2 * kXReq + lane]) : 0u;
        const bool ans = kx >= 0 && fl == (uint32_t)(kx + 1);
        const unsigned long long am = ballot64(ans);
        if (am) {
            agent_acquire();                               // the answer, and the lists and the record behind it
            if (ans) {
                const uint32_t* m = xr + 3 * kXReq + lane * 8;         // (slot, box and list sizes stay there until the cursor comes by)
                const uint32_t res = ld_l2(&m[0]), sn = ld_l2(&m[2]);
                const int r = kx & (RW - 1);
                rg.snap[r] = (uint16_t)sn; rg.aux[r] = (uint32_t)lane;
                st_l2(&xr[2 * kXReq + lane], 0u);
                s_xk[lane] = (res == (uint32_t)R_SKIP || res == (uint32_t)R_REDO) ? -1 : -2;
                st_st(&rg.state[r], (int)res);             // (a release: after the table entries)
            }
            if (lane == 0) atomicSub(&s_xout, __builtin_popcountll(am));
        }
        if (lane == 0) {
            // Help pays where the waves are busy evaluating (an image whose waves wait for the cursor gains nothing from more
            // evaluators): the share of the last ~100 us the waves spent in the idle path below decides whether the image asks
            const int tn = (int)__builtin_amdgcn_s_memtime(), dt = tn - s_xt_last;
            if (dt > 200000) {
                const int ic = lds_ld(&s_idlecnt);
                // ... and only an image that has been running for a while asks at all: at least tun_gate (x 1024 clocks), and at least
                // tun_share percent of the time since the launch began -- the typical image is through before help could pay for the
                // traffic it causes; the ones that have been running for most of the launch are the ones it will end on
                const uint32_t rt_now = (uint32_t)__builtin_amdgcn_s_memrealtime();
                const uint32_t since_launch = rt_now - (ld_l2(&xhdr[4]) & ~1u), mine = rt_now - (uint32_t)rt_begin;
                s_workbound = ((long long)(ic - s_xc_last) * (64 * kWaitSleep + 1000) * 100 < (long long)dt * NW * b.tun_wb &&
                               (long long)__builtin_amdgcn_s_memtime() - t_begin > (long long)b.tun_gate * 1024 &&
                               (unsigned long long)mine * 100ull >= (unsigned long long)since_launch * (unsigned)b.tun_share) ? 1 : 0;   // idle < tun_wb %
                s_xc_last = ic; s_xt_last = tn;
            }
            const int nbg = s_workbound ? max(lds_ld(&s_nbig), 0) : 0;
            s_nhelp = (int)ld_l2(&xr[3]);
            st_l2(&xr[4], (uint32_t)nbg);
            s_xpub = nbg;
            if (!s_xreg && nbg >= NW) {                    // more seeds wait for an evaluation than this workgroup has waves: ask for help
                s_xreg = 1;
                const uint32_t i = atomicAdd(&xhdr[2], 1u);
                st_l2(&xhdr[kXHdr + i], (uint32_t)img + 1u);
            }
        }
        xunlock();
        return am != 0ull;
    };
    // the cursor stands on a seed that was given to the helpers: take the answers in; if nobody has taken the request, take it back
    auto xservice = [&](int f0) -> bool {
        bool moved = false;
        const int r = f0 & (RW - 1);
        if (st_ld(&rg.state[r]) != R_REMOTE || lds_ld(&s_commit) != f0) return true;
        const int j = (int)rg.aux[r];
        int won = 0;
        if (lane == 0) won = atomicCAS(&xr[kXReq + j], (uint32_t)(f0 + 1), 0u) == (uint32_t)(f0 + 1) ? 1 : 0;
        if (__builtin_amdgcn_readfirstlane(won)) {
            if (lane == 0) { s_xk[j] = -1; atomicSub(&s_xout, 1); st_st(&rg.state[r], R_REDO); }
            moved = true;
        }
        return moved;
    };
    // seeds that wait for a full evaluation, the youngest first (the oldest are the local waves'), go to the helpers: at most two
    // requests per helper wavefront outstanding
    auto xexport = [&](int f, int lim) {
        const int nh = lds_ld(&s_nhelp);
        const int cap = min(kXReq - 4, 2 * nh);
        if (nh <= 0 || lim <= f || lds_ld(&s_nbig) <= 0 || lds_ld(&s_xout) >= cap) return;
        if (!xlock()) return;
        for (int it = 0; it < 4; it++) {
            if (lds_ld(&s_nbig) <= 0 || lds_ld(&s_xout) >= cap) break;
            const unsigned long long fm = ballot64(lane < kXReq && s_xk[lane] == -1);
            if (!fm) break;
            const int j = __builtin_ctzll(fm);
            int kb = -1;
            const int b0 = f & ~3;
            for (int base = b0 + ((lim - 1 - b0) & ~255); base >= b0 && kb < 0; base -= 256) {
                const int i0 = base + 4 * lane;
                const uint32_t x = i0 < lim ? __hip_atomic_load(reinterpret_cast<uint32_t*>(rg.state) + ((i0 & (RW - 1)) >> 2), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
                int last = -1;
                #pragma unroll
                for (int t = 0; t < 4; t++)
                    if (((x >> (8 * t)) & 0xffu) == (uint32_t)R_BIG && i0 + t >= f && i0 + t < lim) last = i0 + t;
                const unsigned long long bm = ballot64(last >= 0);
                if (bm) kb = __builtin_amdgcn_readlane(last, 63 - __builtin_clzll(bm));
            }
            if (kb < 0) break;
            int won = 0;
            if (lane == 0) {
                const int r = kb & (RW - 1);
                won = st_cas(rg.state, r, R_BIG, R_EVAL) ? 1 : 0;       // (nobody reads aux of a record in R_EVAL)
                if (won) {
                    atomicSub(&s_nbig, 1); atomicAdd(&s_xout, 1);
                    rg.aux[r] = (uint32_t)j; s_xk[j] = kb;
                    st_st(&rg.state[r], R_REMOTE);
                    st_l2(&xr[kXReq + j], (uint32_t)(kb + 1));
                }
            }
            if (!__builtin_amdgcn_readfirstlane(won)) break;
            STAT(ST_XEXP, 1);
        }
        xunlock();
    };

    // ======== region_image 5/6: seed loop (small-region grower, hand-out, full evaluations) ========
    // Result slots of this wave: slot s holds the lists (and, for a result that marks usedMap, the record in pend[]) of
    // the speculative result of seed slot_k (lane s of slot_k_l); it is free again once the cursor has passed that seed.
    double* const wave_pend = b.pend + (img * NW + wave) * (size_t)NS * 24;
    int slot_k_l = -1;                                     // lane s < NS: seed whose result sits in slot s
    [[maybe_unused]] long long tl = NOW();
    // coarse accounting of this wave's time (s_memtime ticks since the last stamp go to slot i)
#define LT(i) do { const long long t_ = NOW(); DSTAT((i), t_ - tl); tl = t_; } while (0)
    bool adv = false;                                      // a record has been published since the cursor was last looked at

    // ---- The small-region grower: eight seeds side by side ----
    // Nine seeds in ten grow a region of fewer than regThre (12..16) pixels and are dropped at once (:228), and such a region
    // keeps 8 of the 64 lanes of grow() busy.  So the wave's eight 8-lane GROUPS each grow the region of one seed, one list
    // entry x its 8 neighbours per step, out of a private window of 16 x kWinRows packed pixel words around the seed (LDS,
    // loaded once per seed: a small region cannot leave it without being given up first).  The candidates of an entry are
    // decided in reference order against the estimated sum vector exactly as grow() decides a batch pixel by pixel; a test too
    // close to call, a neighbour outside the window or a region that reaches regThre pixels hands the seed over to a full
    // evaluation (R_BIG), which starts from scratch.  A region that reaches its fixpoint first is what RegionGrower returns
    // for that seed, decision for decision; nothing of usedMap is written, so the result is published as R_LIGHT with the
    // box of what it examined.  Groups take the next seed of the wave's chunk as they finish.
    const int grp = lane >> 3, kq = lane & 7;
    const int kk8 = kq + (kq >= 4);                         // 3x3 neighbourhood, row-major, centre skipped (:533-534)
    const int ox = kk8 % 3 - 1, oy = kk8 / 3 - 1;
    int ncap = 1;                                           // a group gives its seed up when the region reaches ncap pixels
    if (g.regThre > 1.0 && g.degThre < 1.5) ncap = g.regThre >= (double)SCAP ? SCAP : (int)ceil(g.regThre);
    const float cos_tol_s = (float)g_tol0[2];
    uint32_t* const swin = G_ARENA(wave) + grp * kWinWords;      // this group's window (the arena holds no full evaluation meanwhile)
    uint32_t* const slst = G_ARENA(wave) + 8 * kWinWords + grp * SCAP;   // this group's list: ly << 4 | lx
    int gk = -1;                                            // seed of this lane's group, -1: idle
    int gn = 0, gi = 0, gex = 0, gsnap = 0;
    float gC = 0.0f, gS = 0.0f;                             // estimated sum vector of the group's region
    int ch_k0 = 0, ch_sx = 0, ch_sy = 0;                    // the wave's chunk: lane j < CH holds seed ch_k0 + j
    unsigned long long ch_pend = 0ull;                      // seeds of the chunk not handed to a group yet
    bool tw_small = false;                                  // the arena holds windows and small lists (not tiles / a region list)
    bool gld = false;                                       // this lane's group waits for its window
    unsigned long long gldm = 0ull;                         // bit 8g: group g waits for its window (wave-uniform)
    int gld_age = 0;                                        // steps since the fetch
// Steps of the small-region groups a wave takes in a row before it goes back to the top of its loop (the cursor, the help protocol, the
// hand-out: ~100 instructions that find nothing new while no group has finished and no window is awaited).  1 / 4 / 16: 31.2 / 30.9 /
// 30.8 ms per step with eight steps in flight (profiles/r06n_inner_steps.log).
#ifndef LSD_REGION_INNER
#define LSD_REGION_INNER 16
#endif
    constexpr int kWinAge = 2; // steps the other groups take before a wave waits for the windows it fetched
    constexpr float kEpsS = 1.0e-5f;                        // kEpsU + the fp32 running sums of up to SCAP unit vectors

    int pend_k = -1, pend_slot = 0;                         // a full evaluation this wave has claimed and starts once its groups are done
    bool pend_spec = false;
    int nwait = 0, wd_f = -1;                               // looks that found nothing to do since the cursor was last seen to move (watchdog)
    long long xlast = 0;                                    // when this wave last looked at the help protocol
    int xwant = 0;                                          // 1: look at the help protocol, 2: ... and the cursor stands on a seed given away
    // The windows fetched at the last refill are in LDS: seeds used meanwhile (:222) are skipped, the others start with their own pixel (:515-520)
    auto window_arrived = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t sw = swin[kSeedRow * 16 + 7];       // (row kSeedRow, column 7 of the window: the seed's own word)
        const bool used = gld && (sw & 3u) != 0u;
        if (gld && !used) {
            float s0, c0;
            fast_sincos(__uint_as_float(sw & ~3u), s0, c0);
            gC = c0; gS = s0; gn = 1; gi = 0; gex = 1;
            if (kq == 0) { swin[kSeedRow * 16 + 7] = sw | 1u; slst[0] = ((uint32_t)kSeedRow << 4) | 7u; }
        }
        if (used) {
            if (kq == 0) st_st(&rg.state[gk & (RW - 1)], R_SKIP);
            gk = -1;
        }
        if (ballot64(used)) adv = true;
        gld = false;
        gldm = 0ull;
        LT(ST_TREFILL);
    };
    while (true) {
        int k = -1, slot = 0;
        bool spec = false;
        if (xwant) {                                       // (the one place the protocol is looked at from: it is a lot of code)
            bool moved = xpoll();
            if (xwant == 2) moved = xservice(lds_ld(&s_commit)) || moved;
            xwant = 0;
            if (moved) adv = true;
        }
        if (adv) {
            // (the cursor is worth a look only when the record it stands on is finished)
            const int f0 = lds_ld(&s_commit);
            const int s0 = f0 < nseeds ? st_ld(&rg.state[f0 & (RW - 1)]) : R_EMPTY;
            LT(ST_TSELECT);
            adv = false;
            if (s0 == R_SKIP || s0 == R_LIGHT || s0 == R_LIGHTL || s0 == R_STASH || s0 == R_XLIGHTL || s0 == R_XSTASH || s0 == R_SETL) advance();
            else if (s0 == R_REMOTE) xwant = 2;
            LT(ST_TCOMMIT);
        }
        LT(ST_TSELECT);
        const unsigned long long actm = ballot64(gk >= 0);
        const int nidle = 8 - __builtin_popcountll(actm & 0x0101010101010101ull);
        bool progress = false;
        int f = 0;
        if (nidle >= (actm ? kFeed : 1)) {
            // ---- feed the idle groups.  Between chunks (the seeds of a chunk are nobody else's) a wave first looks for a full
            //      evaluation to claim; it starts it when the groups still at work have finished ----
            f = lds_ld(&s_commit);
            if (xr && !ch_pend && (lds_ld(&s_nbig) >= NW / 2 || lds_ld(&s_xout) > 0 || lds_ld(&s_xpub) > 0)) {
                // (at most every ~10 us per wave: a look costs an L2 round trip)
                const long long tn = (long long)__builtin_amdgcn_s_memtime();
                if (tn - xlast > b.tun_xpoll) { xlast = tn; xwant = max(xwant, 1); }
            }
            if (!ch_pend && pend_k < 0) {
                const int stf = f < nseeds ? st_ld(&rg.state[f & (RW - 1)]) : R_EMPTY;
                if (stf == R_REDO || stf == R_BIG) {
                    // the record at the cursor: evaluated where everything earlier is committed, no result slot needed
                    int won = 0;
                    if (lane == 0) {
                        won = st_cas(rg.state, f & (RW - 1), stf, R_BUSY) ? 1 : 0;
                        if (won && stf == R_BIG) atomicSub(&s_nbig, 1);
                    }
                    won = __builtin_amdgcn_readfirstlane(won);
                    if (won) { pend_k = f; pend_spec = false; }
                }
                const unsigned long long freem = ballot64(lane < NS && slot_k_l < f);
                if (pend_k < 0 && freem != 0ull && __builtin_popcountll(freem) > NS - max(b.tun_big, min(NS, lds_ld(&s_depth) / (16 * NW))) && lds_ld(&s_nbig) > 0) {   // (tun_big: results a wave may have waiting for the cursor)
                    // the oldest seed waiting for a full evaluation: four records per lane and step
                    const int lim = min(min(lds_ld(&s_next), nseeds), f + lds_ld(&s_depth));
                    int kb = -1;
                    for (int base = f & ~3; base < lim && kb < 0; base += 256) {
                        const int i0 = base + 4 * lane;
                        uint32_t x = i0 < lim ? __hip_atomic_load(reinterpret_cast<uint32_t*>(rg.state) + ((i0 & (RW - 1)) >> 2), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
                        int first = -1;
                        #pragma unroll
                        for (int t = 3; t >= 0; t--)
                            if (((x >> (8 * t)) & 0xffu) == (uint32_t)R_BIG && i0 + t >= f && i0 + t < lim) first = i0 + t;
                        const unsigned long long bm = ballot64(first >= 0);
                        if (bm) kb = __builtin_amdgcn_readlane(first, __builtin_ctzll(bm));
                    }
                    int won = 0;
                    if (lane == 0 && kb >= 0) {
                        const int tgt = kb == lds_ld(&s_commit) ? R_BUSY : R_EVAL;
                        won = st_cas(rg.state, kb & (RW - 1), R_BIG, tgt) ? (tgt == R_BUSY ? 2 : 1) : 0;
                        if (won) atomicSub(&s_nbig, 1);
                    }
                    won = __builtin_amdgcn_readfirstlane(won);
                    if (won) {
                        pend_k = kb; pend_spec = won == 1; pend_slot = __builtin_ctzll(freem);
                        if (pend_spec && lane == pend_slot) slot_k_l = kb;      // the slot is taken until the cursor has passed seed kb
                        progress = true;
                    }
                }
                if (xr && lds_ld(&s_nhelp) > 0 && lds_ld(&s_workbound)) xexport(f, min(min(lds_ld(&s_next), nseeds), f + lds_ld(&s_depth)));
                if (pend_k < 0) {
                    // reserve the next chunk of seeds
                    const int old = lds_ld(&s_next);
                    if (old < nseeds && old + CH - f <= lds_ld(&s_depth)) {
                        int got = 0;
                        if (lane == 0) got = atomicCAS(&s_next, old, old + CH) == old ? 1 : 0;
                        got = __builtin_amdgcn_readfirstlane(got);
                        progress = true;                       // (lost the race: somebody moved, look again)
                        if (got) {
                            ch_k0 = old;
                            const int kx = old + lane;
                            const bool valid = lane < CH && kx < nseeds;
                            uint32_t pp = 0u, code = 1u;
                            if (valid) { pp = seedpos[kx]; code = c.pw[pp] & 3u; }
                            ch_sx = (int)(pp % (uint32_t)w); ch_sy = (int)(pp / (uint32_t)w);
                            const bool used = valid && code != 0u;      // monotone: once used, always used (:222)
                            if (used) st_st(&rg.state[kx & (RW - 1)], R_SKIP);
                            if (ncap <= 1) {
                                // no region is small under these parameters: every seed goes to a full evaluation
                                if (valid && !used) st_st(&rg.state[kx & (RW - 1)], R_BIG);
                                const int nbg = __builtin_popcountll(ballot64(valid && !used));
                                if (lane == 0 && nbg) atomicAdd(&s_nbig, nbg);
                            } else ch_pend = ballot64(valid && !used);
                            adv = true;
                        }
                    }
                }
            }
            // idle groups take the next seeds of the chunk: their windows are FETCHED here (straight into LDS, nothing waits) and the
            // groups start at window_arrived() below, a step or two later -- the round trip to L2 / HBM runs beside the other groups' steps
            const unsigned long long idle0 = ~actm & 0x0101010101010101ull;     // bit 8g: group g is idle
            if (ch_pend && idle0) {
                if (gldm) window_arrived();                // (one fetch in flight at a time)
                unsigned long long idle = idle0;
                const int snap = lds_ld(&s_epoch);         // before anything of usedMap is read for these seeds
                wg_fence();
                tw_small = true;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (the windows' last stores have landed before the fetch may)
                while (idle && ch_pend) {
                    const int j = __builtin_ctzll(ch_pend);
                    ch_pend &= ch_pend - 1ull;
                    const int gg = __builtin_ctzll(idle) >> 3;
                    idle &= idle - 1ull;
                    const int sxj = __builtin_amdgcn_readlane(ch_sx, j), syj = __builtin_amdgcn_readlane(ch_sy, j);
                    if (grp == gg) { gk = ch_k0 + j; gld = true; gsnap = snap; }
                    gldm |= 1ull << (8 * gg);
                    // the window: kWinRows rows of 16 packed pixel words around the seed, as they are in pw[]; lane l < 4 kWinRows fetches quarter l & 3 of row l >> 2
                    const int wx = sxj - 7, wy = syj - kSeedRow;
                    uint32_t* const win = G_ARENA(wave) + gg * kWinWords;
                    const int row = lane >> 2, q4 = (lane & 3) * 4;
                    if (wx >= 0 && wx + 15 < w && wy >= 0 && wy + kWinRows - 1 < h) {
                        // LDS-DMA: lane l's 16 bytes land at M0 + 16 l -- the window's layout
                        const uint32_t* src = c.pw + (size_t)(wy + row) * w + (wx + q4);
                        const uint32_t la = (uint32_t)uni((int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)win);
                        // (M0 is the compiler's to manage and it says so; nothing else in this kernel uses it)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
                        if (kWinRows == 16 || row < kWinRows)   // (the lanes of the rows a shorter window lacks stay out: the next window begins there)
                            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(la), "v"(src) : "memory", "m0");
#pragma clang diagnostic pop
                    } else {
                        const int y = wy + row, x0 = wx + q4;
                        uint32_t v0 = kPwStatic, v1 = kPwStatic, v2 = kPwStatic, v3 = kPwStatic;   // outside the image: banned
                        if ((unsigned)y < (unsigned)h) {
                            const uint32_t* rowp = c.pw + (size_t)y * w;
                            if ((unsigned)(x0 + 0) < (unsigned)w) v0 = rowp[x0 + 0];
                            if ((unsigned)(x0 + 1) < (unsigned)w) v1 = rowp[x0 + 1];
                            if ((unsigned)(x0 + 2) < (unsigned)w) v2 = rowp[x0 + 2];
                            if ((unsigned)(x0 + 3) < (unsigned)w) v3 = rowp[x0 + 3];
                        }
                        if (kWinRows == 16 || row < kWinRows) *reinterpret_cast<uint4*>(&win[lane * 4]) = uint4{v0, v1, v2, v3};
                    }
                }
                gld_age = 0;
                progress = true;
                DSTAT(ST_SLOW, 1);                          // (refill rounds)
                LT(ST_TREFILL);
            }
        }
        if (gldm && (ballot64(gk >= 0 && !gld) == 0ull || ++gld_age >= kWinAge)) window_arrived();
        if (ballot64(gk >= 0)) {
          // (up to kInnerSteps steps in a row while no group finishes and no window is awaited: nothing the top of the loop looks at changes)
          for (int inner = 0; ; inner++) {
            // ---- one step: every active group tests the 8 neighbours of its next list entry ----
            const bool act = gk >= 0 && !gld;
            const uint32_t e = slst[act ? gi : 0];
            const int lx = (int)(e & 15u) + ox, ly = (int)(e >> 4) + oy;
            const bool inwin = ((unsigned)lx < 16u) & ((unsigned)ly < (unsigned)kWinRows);
            const int cell = ((ly & 15) << 4) | (lx & 15);
            const uint32_t word = swin[cell];
            // a neighbour outside the window: the region is not small enough for this grower
            bool bail = ((ballot64(act & !inwin) >> (lane & 56)) & 0xffull) != 0ull;
            bool todo = act & inwin & ((word & 1u) == 0u) & !bail;        // :536-537 (codes 0 and 2 are growable, Q5; a member gets bit 0)
            float sf, cf;
            fast_sincos(__uint_as_float(word & ~3u), sf, cf);
            while (ballot64(todo)) {
                // all candidates still to come, against the estimate as it stands: the ones that clearly fail before the first
                // one that does not are decided for good (nothing is accepted in between); that one must clearly pass
                const float Vg = __builtin_amdgcn_sqrtf(gC * gC + gS * gS) * 1.000001f;
                const float nr = (float)gn * inv_ub(fmaxf(Vg, 1e-3f));
                const float ec = kEpsS * (1.0f + 2.1f * nr) + 5e-6f;
                const float d1 = cf * gC + sf * gS;
                const unsigned long long nfm = ballot64(todo & !(d1 < (cos_tol_s - ec) * Vg));
                const unsigned long long pm = ballot64(d1 > (cos_tol_s + ec) * Vg);
                const uint32_t byte = (uint32_t)(nfm >> (lane & 56)) & 0xffu;
                const bool has = byte != 0u;
                const int l = has ? __builtin_ctz(byte) : 0;
                const int src = (lane & 56) + l;
                const bool acc = has & (((pm >> src) & 1ull) != 0ull);
                // (cos, sin) of the group's lane l in all its lanes: three DPP steps each instead of a round trip through the LDS crossbar
                const float cl = sum8(kq == l ? cf : 0.0f);
                const float sl = sum8(kq == l ? sf : 0.0f);
                if (acc & (kq == l)) {
                    swin[cell] = word | 1u;                                   // :549
                    slst[gn] = (uint32_t)((ly << 4) | lx);                   // :551-556
                }
                gC += acc ? cl : 0.0f; gS += acc ? sl : 0.0f;                // :545-546 (estimate)
                gn += acc ? 1 : 0;
                bail = bail | (has & !acc) | (acc & (gn >= ncap));            // too close to call / not a small region
                todo = todo & acc & !bail & (kq > l);
            }
            const int ni = gi + 1;
            const bool sweep_end = act & !bail & (ni >= gn);                  // :529 (the list is live)
            const bool done = sweep_end & (gn == gex);                       // :525 a sweep that added nothing
            gex = sweep_end ? gn : gex;
            gi = sweep_end ? 0 : ni;
            const bool fin = act & (done | bail);
            const unsigned long long finm = ballot64(fin & (kq == 0));
            if (finm) {
                // box of the list's pixels, relative to the seed (window cell 7, kSeedRow): what a line accepted before the seed's turn must not touch
                const uint32_t e0 = slst[kq < gn ? kq : 0], e1 = slst[kq + 8 < gn ? kq + 8 : 0];
                const int bx0 = imin8(min((int)(e0 & 15u), (int)(e1 & 15u))), bx1 = imax8(max((int)(e0 & 15u), (int)(e1 & 15u)));
                const int by0 = imin8(min((int)(e0 >> 4), (int)(e1 >> 4))), by1 = imax8(max((int)(e0 >> 4), (int)(e1 >> 4)));
                const bool light = fin & !bail;
                if (fin & (kq == 0)) {
                    const int r = gk & (RW - 1);
                    if (light) {
                        rg.snap[r] = (uint16_t)gsnap;
                        rg.aux[r] = (uint32_t)(bx0 - 7 + 32) | ((uint32_t)(by0 - kSeedRow + 32) << 6) | ((uint32_t)(bx1 - 7 + 32) << 12) | ((uint32_t)(by1 - kSeedRow + 32) << 18);
                        if (trace) { rnum[r * 2] = gn; rnum[r * 2 + 1] = gn << 2; }
                    }
                    st_st(&rg.state[r], light ? R_LIGHT : R_BIG);
                }
                const unsigned long long lightm = ballot64(light & (kq == 0));
                const int nbg = __builtin_popcountll(finm & ~lightm);
                if (lane == 0 && nbg) atomicAdd(&s_nbig, nbg);
                int gsum = 0;
                for (unsigned long long t = lightm; t; t &= t - 1ull) gsum += __builtin_amdgcn_readlane(gn, __builtin_ctzll(t));
                STAT(ST_GROW, __builtin_popcountll(lightm)); STAT(ST_GROWN, gsum); DSTAT(ST_SMALLBAIL, nbg);
                gk = fin ? -1 : gk;
                adv = true;
            }
            DSTAT(ST_SMALLSTEPS, 1);
            if (finm || gldm || inner >= LSD_REGION_INNER - 1) break;
          }
            LT(ST_TSMALL);
            nwait = 0;
            continue;
        }
        if (pend_k >= 0) { k = pend_k; spec = pend_spec; slot = pend_slot; pend_k = -1; nwait = 0; }
        else {
            if (progress) { nwait = 0; continue; }
            if (lds_ld(&s_next) >= nseeds && lds_ld(&s_commit) >= nseeds) break;   // everything is committed
            // Watchdog: the protocol has no state in which every wave waits; should one arise all the same (a defect), the image
            // is given up after seconds of nobody moving instead of hanging the device: counts[img] = -1, the state goes to stats.
            {   // (the cursor as this wave last saw it is kept across looks: movement during the sleep below, or by this wave's own
                //  advance() at the top of the next look, counts)
                const int fc = lds_ld(&s_commit);
                if (fc != wd_f) { wd_f = fc; nwait = 0; }
            }
            if (++nwait > LSD_REGION_WATCHDOG || lds_ld(&s_abort)) {
                if (b.stats && lane == 0) {
                    long long* st = b.stats + img * kStatWords;
                    if (!lds_ld(&s_abort)) {
                        const int fc = lds_ld(&s_commit);
                        st[40] = fc; st[41] = lds_ld(&s_next); st[42] = nseeds; st[43] = fc < nseeds ? st_ld(&rg.state[fc & (RW - 1)]) : -1;
                        st[44] = lds_ld(&s_nbig); st[45] = lds_ld(&s_lock); st[46] = pend_k; st[47] = wave;
                    }
                    st[24 + 2 * wave] = (long long)ch_k0 | ((long long)(pend_k + 1) << 32);     // what this wave holds (developer record)
                    st[25 + 2 * wave] = (long long)ch_pend;
                }
                if (lane == 0) lds_st(&s_abort, 1);
                break;
            }
            // within the look-ahead there is nothing for this wave (no seed to hand out, no evaluation to claim): look further
            if (nwait == 1 && lane == 0 && lds_ld(&s_next) < nseeds) {
                const int d = lds_ld(&s_depth);
                if (d < depth_max) lds_st(&s_depth, min(d + kDepthUp, depth_max));
            }
            // nothing to do: every slot waits for the cursor, the ring is full, or nothing is left to hand out.  Sleep long
            // enough that the polling of the waiting waves does not take issue slots from the evaluation the cursor waits for
            if (lds_ld(&s_commit) == f) __builtin_amdgcn_s_sleep(kWaitSleep);
            if (xr) { if (lane == 0) atomicAdd(&s_idlecnt, 1); if (lds_ld(&s_xout) > 0) xwant = max(xwant, 1); }   // answers of the helpers
            adv = true;                                    // (look at the cursor again before asking for a job)
#ifdef LSD_REGION_STATS
            {   // why this wave had nothing to do: no result slot for a waiting seed / the ring is full / no seed is left
                const int old = lds_ld(&s_next);
                const long long t_ = NOW();
                const int why = old >= nseeds ? ST_WNOSEED : (lds_ld(&s_nbig) > 0 ? ST_WNOSLOT : ST_WAIT);
                DSTAT(why, t_ - tl); tl = t_;
            }
#else
            LT(ST_WAIT);
#endif
            continue;
        }
        // ---- a full evaluation of seed k (RegionGrower ... RectangleImprover with all 64 lanes) ----
        const uint32_t pp = seedpos[k];

        // ---- evaluate ----
        const int epoch_snap = lds_ld(&s_epoch);           // before anything of usedMap is read for this seed
        wg_fence();
        if (tw_small || !spec || epoch_snap != g_ws[wave].cache_epoch) {   // tiles fetched before the last accept may miss its bans
            invalidate_tiles(c);
            g_ws[wave].cache_epoch = epoch_snap;
            tw_small = false;
        }
        eval_seed(c.wave, pp, spec ? 1 : 0, slot);
#ifdef LSD_REGION_INJECT_STALL
        if (img & 1) continue;                             // test build (make wdtest): odd images never publish a full evaluation -> the watchdog has to end them
#endif
        const EvalOut& eo = g_eo[wave];
        const bool skip = eo.skip != 0;
        const int outcome = eo.outcome, num = eo.num, num0 = eo.num0, rec_pk = eo.rec_pk;
        const double logNFA = eo.logNFA;
        const double pv = lane < 12 ? reinterpret_cast<const double*>(&g_ws[wave].rec)[lane] : 0.0;   // lane j < 12: field j of the result's rectangle (structRec order)

        // ---- hand the result over ----
#ifdef LSD_REGION_STATS
        if (!spec) DSTAT(ST_DEPTHDN, NOW() - tl);          // (time of the evaluations AT the cursor: everybody else may be waiting for them)
#endif
        LT(ST_TEVAL);
        if (!spec) {
            // ---- evaluated at the cursor (k == s_commit, record R_BUSY: nobody else can commit): commit right away ----
            if (!skip && outcome >= 2) {
                // (under the cursor lock although nobody else can commit here: certify_set() relies on no ban appearing while it holds it)
                while (true) {
                    int got = 0;
                    if (lane == 0) got = atomicCAS(&s_lock, 0, 1) == 0 ? 1 : 0;
                    if (__builtin_amdgcn_readfirstlane(got)) break;
                    __builtin_amdgcn_s_sleep(2);
                }
                commit_marks(k, num0, num, outcome, logNFA, pv, nullptr, 0);
                if (lane == 0) lds_st(&s_lock, 0);
            }
            else if (!skip) write_trace(k, num0, outcome == 0 ? num0 : num, outcome, logNFA);
            wg_fence();
            if (lane == 0) { rg.state[k & (RW - 1)] = (uint8_t)R_EMPTY; lds_st(&s_commit, k + 1); }
            LT(ST_TCOMMIT);
            adv = true;
            continue;
        }
        if (skip) {
            if (lane == slot) slot_k_l = -1;               // nothing kept in the slot
            if (lane == 0) st_st(&rg.state[k & (RW - 1)], R_SKIP);
            adv = true;
            continue;
        }
        if (eo.setid) {                                    // answered by a certified set: nothing is kept in the slot
            if (lane == slot) slot_k_l = -1;
            if (lane == 0) {
                const int r = k & (RW - 1);
                rg.snap[r] = (uint16_t)epoch_snap;
                rg.aux[r] = (uint32_t)eo.setid;
                if (trace) { rnum[r * 2] = num0; rnum[r * 2 + 1] = (num << 2) | outcome; }
                st_st(&rg.state[r], R_SETL);
            }
            adv = true;
            continue;
        }
        const int x0 = eo.x0, y0 = eo.y0, x1 = eo.x1, y1 = eo.y1, n1 = eo.n1, n2 = eo.n2, m_off = eo.m_off, mcnt = eo.mcnt;
        const bool precise = eo.precise != 0, redo = eo.redo != 0;
        if (outcome <= 1) {                                // nothing to mark: publish and move on
            if (lane == 0) {
                const int r = k & (RW - 1), si = wave * NS + slot;
                rg.snap[r] = (uint16_t)epoch_snap;
                rg.aux[r] = (uint32_t)si;
                stab.box[si][0] = (short)x0; stab.box[si][1] = (short)y0; stab.box[si][2] = (short)x1; stab.box[si][3] = (short)y1;
                stab.lcnt[si] = precise ? ((uint32_t)(n1 + 1) | ((uint32_t)n2 << 16)) : 0u;
                if (trace) { rnum[r * 2] = num0; rnum[r * 2 + 1] = (num << 2) | outcome; }
            }
            wg_fence();                                    // the lists are in the slot before the record says so
            if (lane == 0) st_st(&rg.state[k & (RW - 1)], R_LIGHTL);
            adv = true;
            // an evaluation that went the way of a uniform set offers its first list (still in the slot) as a certified set
            if (eo.cert && certify_set(c.wave, pp, slot, num0, &s_lock, &s_nsets)) STAT(ST_SETNEW, 1);
            continue;
        }
        // marks to make: the result is stashed (record in pend[], the pixels to mark in the list slot); whoever moves the
        // cursor over it commits it
        if (redo) {
            if (lane == 0) st_st(&rg.state[k & (RW - 1)], R_REDO);
            STAT(ST_REDO, 1);
            adv = true;
            continue;
        }
        if (lane < 12) wave_pend[slot * 24 + lane] = pv;
        if (lane == 0) {
            double* P = wave_pend + slot * 24;
            P[12] = logNFA;
            P[13] = (double)rec_pk; P[14] = (double)outcome; P[15] = (double)num0; P[16] = (double)num; P[17] = (double)mcnt;
            P[18] = (double)x0; P[19] = (double)y0; P[20] = (double)x1; P[21] = (double)y1;
            P[22] = (double)((long long)(precise ? n1 + 1 : 0) + 32768ll * n2 + 32768ll * 32768ll * m_off);
            P[23] = (double)epoch_snap;
            rg.aux[k & (RW - 1)] = (uint32_t)(wave * NS + slot);
        }
        wg_fence();                                        // record and lists are in the slot before the ring says so
        if (lane == 0) st_st(&rg.state[k & (RW - 1)], R_STASH);
        adv = true;
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (an image given up by the watchdog may leave a window fetch in flight: nothing lands in LDS after the wave is gone)
    // ---- this image is finished (every seed committed, or given up): results out ----
    if (wave == 0 && lane == 0 && !pool) {
        b.counts[img] = lds_ld(&s_abort) ? -1 : s_lines;
        if (b.nseed) b.nseed[img] = s_ntrace;
    }
    if (b.stats && !pool) {
        unsigned long long* st = reinterpret_cast<unsigned long long*>(b.stats + img * kStatWords);
        if (lane == 0 && wave == 0 && !lds_ld(&s_abort)) { atomicAdd(&st[kStatGrowAnyWord], (unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15)); b.stats[img * kStatWords + 46] = rt_begin; b.stats[img * kStatWords + 47] = (long long)__builtin_amdgcn_s_memrealtime(); }   // (developer record: when the image ran)
        if (lane == 0 && wave == 0) {
            // shader clocks of this workgroup on the image.  s_memtime is a counter of the XCD the wavefront runs on: a workgroup that was
            // preempted (more hardware queues in use than the device has -- e.g. two processes with 16 each -- make the scheduler time-slice
            // them, saving and restoring wavefronts) and resumed on another XCD reads another counter, and the difference comes out negative or
            // absurd (seen in the test suite, which starts bench.py beside its own process).  Then the constant 100 MHz clock stands in, at the
            // nominal 24 shader clocks per tick.
            long long tot = (long long)__builtin_amdgcn_s_memtime() - t_begin;
            const long long rt = ((long long)__builtin_amdgcn_s_memrealtime() - rt_begin) * 24;
            if (tot <= 0 || tot > 4 * rt + 1000000) tot = rt > 0 ? rt : 1;
            g_stat[c.wave][sslot(ST_TOTAL)] = (unsigned long long)tot; g_stat[c.wave][sslot(ST_SEEDS)] = (unsigned long long)nseeds; DSTAT(ST_DEPTHEND, lds_ld(&s_depth));
        }
        if (lane < ST_COUNT && !lds_ld(&s_abort) && (sslot(lane) != 11 || lane == ST_NFASLOW || kStatSlots > ST_COUNT)) {   // (kStatSlots > ST_COUNT: the developer build, a slot per counter)
            if (lane == ST_MINNFA || lane == ST_MINGAP) atomicMax(&st[lane], g_stat[c.wave][sslot(lane)]);
            else atomicAdd(&st[lane], g_stat[c.wave][sslot(lane)]);
        }
        if (lane == 0 && !lds_ld(&s_abort)) atomicAdd(&st[kStatGrowAnyWord], g_stat[c.wave][sslot(ST_GROWANY)] << 8);   // (the record starts from zero: the XCC above and the waves' counts add up in any order)
        g_stat[c.wave][sslot(ST_XHELP)] = 0ull;
        // (what a helper adds to ANOTHER image's record below starts from zero: not from this image's own margins and ties)
        g_stat[c.wave][sslot(ST_MINNFA)] = 0ull; g_stat[c.wave][sslot(ST_MINGAP)] = 0ull; g_stat[c.wave][sslot(ST_NFASLOW)] = 0ull; g_stat[c.wave][sslot(ST_TIES)] = 0ull;
    }
    if (!b.xq) return;
    if (wave == 0 && !pool) {
        agent_release();
        if (lane == 0) { st_l2(&xr[2], 1u); atomicAdd(&xhdr[1], 1u); }
    }
    // While workgroups still wait for a CU this one should make room -- unless an image is so far behind with its evaluations
    // that a few wavefronts are better spent there (EARLY helpers: at most tun_early workgroups' worth at a time, only for images
    // with two backlogged seeds per wave of their own, and gone as soon as there is nothing of that kind)
    bool early = !pool && ld_l2(&xhdr[0]) < (uint32_t)nimg;
    if (early) {
        if (b.tun_early <= 0) return;
        int ok = 0;
        if (lane == 0) {
            if (atomicAdd(&xhdr[3], 1u) >= (uint32_t)(b.tun_early * NW)) atomicSub(&xhdr[3], 1u);
            else ok = 1;
        }
        if (!__builtin_amdgcn_readfirstlane(ok)) return;
    }

    // ======== region_image 6/6: helper loop ========
    // ---- ... then help elsewhere: every wavefront on its own (see "Help from other workgroups" above) ----
    if (lane < NS) slot_k_l = -1;
    int hx = -1, hj = 0, hidle = 0, hscan = 0;              // image this wave helps (-1: none), request it is answering, looks without work / for an image
    uint32_t* hrec = nullptr;                               // that image's record of the help protocol
    const uint32_t* cur_seedpos = seedpos;
    // the work counters of an evaluation done for another image (grows, grown pixels, NFA and RegionRadiusReducer calls: slots 0..6)
    // go to THAT image's record, as if its own waves had done it
    unsigned long long hprev = lane < 7 ? g_stat[c.wave][lane] : 0ull;
    while (true) {
        int k = -1, slot = 0;
        if (hx < 0) {
            // ---- not attached: the image with the largest backlog per wave already working on it ----
            if (ld_l2(&xhdr[1]) >= (uint32_t)nimg) break;   // every image is finished
            if (early && ld_l2(&xhdr[0]) >= (uint32_t)nimg) {   // every workgroup has its CU by now
                early = false;
                if (lane == 0) atomicSub(&xhdr[3], 1u);
            }
            const int wt = min(min((int)ld_l2(&xhdr[2]), nimg), 4096);
            uint32_t best = 0u;
            for (int base = 0; base < wt; base += 64) {
                const int i = base + lane;
                uint32_t key = 0u;
                if (i < wt) {
                    const uint32_t im1 = ld_l2(&xhdr[kXHdr + i]);
                    if (im1) {
                        const uint32_t* rc = b.xq + (size_t)(im1 - 1u) * kXStride;
                        if (!ld_l2(&rc[2])) {
                            const uint32_t bl = ld_l2(&rc[4]), nh = ld_l2(&rc[3]);
                            if (bl >= (early ? 2u * NW : 1u) && nh < (uint32_t)(early ? NW : b.tun_help)) key = ((min(bl * 16u / (nh + NW), 0xffffeu) + 1u) << 12) | (uint32_t)i;
                        }
                    }
                }
                #pragma unroll
                for (int o = 32; o; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o));
                best = max(best, key);
            }
            best = (uint32_t)uni((int)best);
            if (!best) {
                if (early) { if (lane == 0) atomicSub(&xhdr[3], 1u); break; }
                if (++hscan > b.tun_linger) break;         // nobody has asked for a while: give the CU back (another launch may be waiting for it)
                for (int t = 0; t < 8; t++) __builtin_amdgcn_s_sleep(127);
                continue;
            }
            const uint32_t im = ld_l2(&xhdr[kXHdr + (best & 4095u)]) - 1u;
            uint32_t* rc = b.xq + (size_t)im * kXStride;
            int ok = 0;
            if (lane == 0) {
                if (atomicAdd(&rc[3], 1u) >= (uint32_t)(early ? NW : b.tun_help)) atomicSub(&rc[3], 1u);
                else ok = 1;
            }
            if (!__builtin_amdgcn_readfirstlane(ok)) continue;
            hx = (int)im; hrec = rc; hidle = 0; hscan = 0;
            cur_seedpos = b.seedpos + (size_t)im * npx;
            c.mag = b.mag + (size_t)im * npx; c.deg = b.deg + (size_t)im * npx; c.pw = b.pw + (size_t)im * npx;
            c.epochmap = b.epochmap + (size_t)im * npx; c.sc = b.sc + (size_t)im * npx; c.sets = nullptr;
            c.tep = b.tepoch + (size_t)im * (size_t)(((w + 7) >> 3) * ((h + 7) >> 3));
            if (lane == 0) {
                RCtx& gc = g_ctx[wave];
                gc.mag = c.mag; gc.deg = c.deg; gc.pw = c.pw; gc.epochmap = c.epochmap; gc.sc = c.sc; gc.tep = c.tep; gc.sets = nullptr;
                g_ws[wave].cache_epoch = -1;
            }
            wg_fence();
            continue;
        }
        // ---- attached to image hx: a request to answer ----
        const uint32_t cm = ld_l2(&hrec[1]);
        const bool xdone = ld_l2(&hrec[2]) != 0u;
        if (lane < NS && (xdone || slot_k_l < (int)cm)) slot_k_l = -1;          // the cursor has passed these results
        const unsigned long long freem = ballot64(lane < NS && slot_k_l < 0);
        if (xdone || (hidle > kHelpIdle && freem == (1ull << NS) - 1ull)) {
            if (lane == 0) atomicSub(&hrec[3], 1u);
            hx = -1;
            continue;
        }
        if (__builtin_popcountll(freem) <= NS - b.tun_big) { __builtin_amdgcn_s_sleep(127); continue; }   // (as for local waves)
        const uint32_t rq = lane < kXReq ? ld_l2(&hrec[kXReq + lane]) : 0u;
        uint32_t key = (rq != 0u && (rq >> 31) == 0u) ? rq : 0xffffffffu;          // the oldest seed first
        #pragma unroll
        for (int o = 32; o; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o));
        key = (uint32_t)uni((int)key);
        if (key == 0xffffffffu) { hidle++; __builtin_amdgcn_s_sleep(127); continue; }
        const int jj = __builtin_ctzll(ballot64(rq == key));
        int ok = 0;
        if (lane == 0) ok = atomicCAS(&hrec[kXReq + jj], key, key | 0x80000000u) == key ? 1 : 0;
        if (!__builtin_amdgcn_readfirstlane(ok)) continue;
        k = (int)key - 1; slot = __builtin_ctzll(freem); hj = jj; hidle = 0;
        if (lane == slot) slot_k_l = k;
        const uint32_t pp = cur_seedpos[k];
        const int epoch_snap = (int)ld_l2(&hrec[0]);       // before anything of usedMap is read for this seed ...
        agent_acquire();                                   // ... (the acquire empties this CU's L1: the bans made up to that epoch are seen)
        if (epoch_snap != g_ws[wave].cache_epoch) {         // tiles fetched before the last accept may miss its bans
            invalidate_tiles(c);
            g_ws[wave].cache_epoch = epoch_snap;
        }
        eval_seed(c.wave, pp, 1, slot);
        if (b.stats && lane < 7) {
            const unsigned long long v = g_stat[c.wave][lane];
            if (v != hprev) atomicAdd(reinterpret_cast<unsigned long long*>(b.stats + (size_t)hx * kStatWords) + lane, v - hprev);
            hprev = v;
        }
        if (b.stats && lane == 0) {                        // ... and how close its NFA comparisons came to a tie
            unsigned long long* const hs = reinterpret_cast<unsigned long long*>(b.stats + (size_t)hx * kStatWords);
            atomicMax(&hs[ST_MINNFA], g_stat[c.wave][sslot(ST_MINNFA)]); atomicMax(&hs[ST_MINGAP], g_stat[c.wave][sslot(ST_MINGAP)]);
            atomicAdd(&hs[ST_NFASLOW], g_stat[c.wave][sslot(ST_NFASLOW)]);
            atomicAdd(&hs[ST_TIES], g_stat[c.wave][sslot(ST_TIES)]);
        }
        if (b.stats) { g_stat[c.wave][sslot(ST_MINNFA)] = 0ull; g_stat[c.wave][sslot(ST_MINGAP)] = 0ull; g_stat[c.wave][sslot(ST_NFASLOW)] = 0ull; g_stat[c.wave][sslot(ST_TIES)] = 0ull; }
        const EvalOut& eo = g_eo[wave];
        const bool skip = eo.skip != 0;
        const int outcome = eo.outcome, num = eo.num, num0 = eo.num0, rec_pk = eo.rec_pk;
        const double logNFA = eo.logNFA;
        const double pv = lane < 12 ? reinterpret_cast<const double*>(&g_ws[wave].rec)[lane] : 0.0;
        // the answer: what a local evaluation would have published, with the lists (and the record) in this wave's slot
        const bool xredo = !skip && outcome >= 2 && eo.redo != 0;
        const int res = skip ? R_SKIP : outcome <= 1 ? R_XLIGHTL : xredo ? R_REDO : R_XSTASH;
        const size_t my_slot = (img * NW + wave) * (size_t)NS + slot;
        if (res == R_XSTASH) {
            double* P = b.pend + my_slot * 24;
            if (lane < 12) P[lane] = pv;
            if (lane == 0) {
                P[12] = logNFA;
                P[13] = (double)rec_pk; P[14] = (double)outcome; P[15] = (double)num0; P[16] = (double)num; P[17] = (double)eo.mcnt;
                P[18] = (double)eo.x0; P[19] = (double)eo.y0; P[20] = (double)eo.x1; P[21] = (double)eo.y1;
                P[22] = (double)((long long)(eo.precise ? eo.n1 + 1 : 0) + 32768ll * eo.n2 + 32768ll * 32768ll * eo.m_off);
                P[23] = (double)epoch_snap;
            }
        }
        if (res == R_SKIP || res == R_REDO) { if (lane == slot) slot_k_l = -1; }      // nothing kept in the slot
        if (lane == 0) {
            uint32_t* m = hrec + 3 * kXReq + hj * 8;
            st_l2(&m[0], (uint32_t)res); st_l2(&m[1], (uint32_t)my_slot); st_l2(&m[2], (uint32_t)epoch_snap);
            if (res == R_XLIGHTL) {
                st_l2(&m[3], (uint32_t)(eo.x0 & 0xffff) | ((uint32_t)(eo.y0 & 0xffff) << 16));
                st_l2(&m[4], (uint32_t)(eo.x1 & 0xffff) | ((uint32_t)(eo.y1 & 0xffff) << 16));
                st_l2(&m[5], eo.precise ? ((uint32_t)(eo.n1 + 1) | ((uint32_t)eo.n2 << 16)) : 0u);
            }
        }
        agent_release();                               // lists, record and message before the flag
        if (lane == 0) st_l2(&hrec[2 * kXReq + hj], (uint32_t)(k + 1));
        STAT(ST_XHELP, 1);
        continue;
    }
    // (a helper's count of evaluations done for others goes to its own image's record)
    if (b.stats && lane == 0 && !pool) atomicAdd(reinterpret_cast<unsigned long long*>(b.stats + img * kStatWords) + ST_XHELP, g_stat[c.wave][sslot(ST_XHELP)]);
}
#undef LT

// K5 by the workgroup that has just finished the image at place `bid` of the launch's order (b.fuse_lines; lsd_ctx.hip says when): the
// records of its accepted rectangles are final, so their lines are written here, by all of its wavefronts, instead of by a kernel behind
// the whole launch -- one dispatch less per step, and an image's lines no longer wait for the slowest image of the batch.  Out of line,
// called from the kernel function with nothing of the image's own state live any more: the kernel body's register allocation is
// untouched (DESIGN_NOTES.md, "the lean kernel body").  The caller has passed a barrier since the image's last commit: the records
// and the count, written by whichever wavefront moved the cursor, are visible to all of the workgroup's.
// (The arguments one by one, not the Buffers record: a reference to it would make the kernel keep a copy of its arguments in scratch.)
__device__ __noinline__ void region_lines(const uint32_t* order, const int32_t* counts, const double* recs_scaled, lsd_line* lines, uint8_t* line_im,
                                          int max_lines, int W, int H, int bid) {
    const size_t img = order[bid];
    const int count = __hip_atomic_load(&counts[img], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    lines_of_image(recs_scaled + img * (size_t)max_lines * 4, count, lines + img * (size_t)max_lines,
                   line_im ? line_im + img * (size_t)W * H : nullptr, max_lines, W, H, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63), NW);
}

// The launch.  One workgroup per image (+ b.npool helper-only workgroups), dispatched in the order of k_order -- or, on the 8-wave
// build, PERSISTENT workgroups (b.pcount, lsd_ctx.hip: a batch of more images than the device has CUs, help off): as many workgroups
// as CUs, each taking the next image of that order from the launch's counter until none is left.  The hardware deals the workgroups
// of a launch onto the eight XCDs round-robin and never moves them, so with one workgroup per image an XCD whose 64 images are heavy
// finishes last while CUs of the others idle; the counter balances across XCDs: 512 maps as one step 78.6 -> 73.4 ms
// (profiles/r06d_scheduling_probes.log).  Not for the 4-wave build: there the loop around the image's code costs the kernel body's register
// allocation 16 % (31.3 -> 36.4 ms per step with eight steps in flight, same log) and buys nothing (persistent workgroups let the
// front ends of the other steps flow -- their dispatches no longer wait behind a launch that does not fit the device -- but the steps'
// tails leave the slots of finished workgroups empty: 36.6-45.7 ms against 36.8).
__global__ __launch_bounds__(64 * NW, LSD_REGION_WAVES_PER_SIMD) void k_region(Geom g, Buffers b, uint32_t id_base) {
#if LSD_REGION_NW == 8
    __shared__ int s_take;
    while (true) {                                          // (one call site: the image's code exists once)
        int bid = (int)blockIdx.x, nimg = (int)gridDim.x - b.npool;
        if (b.pcount) {
            if (threadIdx.x == 0) s_take = atomicAdd(b.pcount, 1);
            __syncthreads();
            bid = s_take; nimg = b.nimg;
            __syncthreads();                                // (everybody has read it before the next round overwrites it)
            if (bid >= nimg) return;
        }
        region_image(g, b, id_base, bid, nimg);
        if (b.fuse_lines) { __syncthreads(); region_lines(b.order, b.counts, b.recs_scaled, b.lines, b.line_im, b.max_lines, g.W, g.H, bid); }   // (never with help across workgroups: every workgroup owns an image and all its wavefronts arrive)
        if (!b.pcount) return;
        __syncthreads();                                    // every wavefront is out of the image before its shared state is set up again
    }
#else
    region_image(g, b, id_base, (int)blockIdx.x, (int)gridDim.x - b.npool);
    if (b.fuse_lines) { __syncthreads(); region_lines(b.order, b.counts, b.recs_scaled, b.lines, b.line_im, b.max_lines, g.W, g.H, (int)blockIdx.x); }
#endif
}

}  // namespace RVAR

#if LSD_REGION_NW == 8
void launch_region_w8(const Geom& g, const Buffers& b, int n, uint32_t id_base, hipStream_t s) {
    hipLaunchKernelGGL(w8::k_region, dim3(n + b.npool), dim3(64 * w8::NW), 0, s, g, b, id_base);
}
// workspace is sized for the wider variant
int region_slots() { return w8::NS; }
int region_waves() { return w8::NW; }
int region_ring() { return w8::RW; }
#else
void launch_region_w4(const Geom& g, const Buffers& b, int n, uint32_t id_base, hipStream_t s) {
    hipLaunchKernelGGL(w4::k_region, dim3(n + b.npool), dim3(64 * w4::NW), 0, s, g, b, id_base);
}
#endif

}  // namespace lsdhip
