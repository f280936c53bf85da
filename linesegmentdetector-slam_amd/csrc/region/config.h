// region/config.h -- build configuration of the region stage (part of k_region.hip, included inside its variant namespace): the LSD_REGION_* defaults and the
// sizes derived from them, the labels of certified sets, and the records every stage shares: Rec (structRec, myLSD.h:80-93), WState, RCtx.  Declares no LDS object.
#ifndef LSD_REGION_WAVES_PER_SIMD
#define LSD_REGION_WAVES_PER_SIMD 2
#endif
#ifndef LSD_REGION_NS
#define LSD_REGION_NS 16
#endif
constexpr int kWaitSleep = 127;         // s_sleep of a wave that found nothing to do, x 64 clocks
#ifndef LSD_REGION_WATCHDOG
#define LSD_REGION_WATCHDOG 600000     // looks of one wave (a sleep of kWaitSleep x 64 clocks, ~3.4 us, each) that found nothing to do
                                       // while the cursor, as that wave saw it, never moved
#endif
constexpr int NW = LSD_REGION_NW;        // wavefronts (concurrent speculative seeds) per image
constexpr int NS = LSD_REGION_NS;        // result slots per wave: seeds a wave may have evaluated ahead of the cursor
// Four workgroups per CU (LSD_REGION_WAVES_PER_SIMD >= 4 on the 4-wave build) leave each 40 KB of LDS: the build then takes the small sizes
// below.  Every one of them only moves the point at which an existing, slower path with the same answer is taken (a small region handed to a
// full evaluation, a list written through to `spill`, one more round of staging), so the committed sequence is the same at either size.
#if LSD_REGION_WAVES_PER_SIMD >= 4
#define LSD_REGION_DIET 1
#else
#define LSD_REGION_DIET 0
#endif
#ifndef LSD_REGION_LCAP
#define LSD_REGION_LCAP (LSD_REGION_DIET ? 256 : 512)
#endif
#ifndef LSD_REGION_WINROWS
#define LSD_REGION_WINROWS (LSD_REGION_DIET ? 12 : 16)
#endif
#ifndef LSD_REGION_STAGE
#define LSD_REGION_STAGE (LSD_REGION_DIET ? 16 : 32)
#endif
#ifndef LSD_REGION_NT
#define LSD_REGION_NT 16
#endif
// The region list of a grow lives in LDS as a RING of the LCAP entries appended last (slot = index mod LCAP): the sweep that appends
// entries reads them again a frontier's width later, which for the thin structures of an occupancy map is a handful of entries,
// whatever the length of the region.  A list that outgrows the ring is also written through to HBM (`spill`, all entries, from the
// moment the ring would wrap), where the few readers of older entries find them (re-sweeps, the sums over the whole list).
constexpr int LCAP = LSD_REGION_LCAP;   // entries of the list ring (a power of two)
constexpr int LMASK = LCAP - 1;
constexpr int NT = LSD_REGION_NT;       // tile-cache slots per wave (8x8-pixel tiles of packed pixel words; a power of two; 16 measured as good as 32)
static_assert((NT & (NT - 1)) == 0 && NT >= 8 && LCAP >= 256 && (LCAP & (LCAP - 1)) == 0, "tile slots and list ring: powers of two");
// The small-region grower's window: 16 columns x kWinRows rows of packed pixel words with the seed in column 7 of row kSeedRow (16 rows: 7 above the
// seed and 8 below; 12 rows: 5 and 6).  A region whose examined pixels leave the window goes to a full evaluation.
constexpr int kWinRows = LSD_REGION_WINROWS;
constexpr int kSeedRow = (kWinRows - 1) / 2;
constexpr int kWinWords = 16 * kWinRows;
static_assert(kWinRows >= 8 && kWinRows <= 16 && (kWinRows & 3) == 0, "window rows: a multiple of four (lane l fetches a quarter of row l >> 2), at most 16 (list entries are ly << 4 | lx)");
constexpr int kStage = LSD_REGION_STAGE;   // list elements the serial sums stage per round (lds.h: stage4 / acc32)
static_assert(kStage == 16 || kStage == 32, "staging rounds of 16 or 32 elements");
constexpr int RING = 128;    // remembered bounding boxes of recently accepted lines
constexpr int kSetMax = 255;           // certified sets per image and launch (labels 1 .. kSetMax)
constexpr int kSetMinPixels = 64;      // ... of at least this many pixels
constexpr uint32_t kSetPending = 0x80000000u;
// The label of a growable pixel (in its epochmap word): bit 31 | the launch's tag << 8 | set number.  Accept epochs (small integers) and
// the labels of earlier launches in the same buffers never look like one of THIS launch (the tag is the run number, as for the stamps).
__device__ __forceinline__ uint32_t label_make(uint32_t tag, uint32_t id) { return 0x80000000u | (tag << 8) | id; }
__device__ __forceinline__ uint32_t label_set(uint32_t tag, uint32_t word) { return (word >> 8) == (0x800000u | tag) ? (word & 0xffu) : 0u; }

struct Rec {  // structRec, myLSD.h:80-93 (+ pk = number of halvings of p, indexes the host log tables)
    double x1, y1, x2, y2, wid, cX, cY, deg, dx, dy, p, prec;
    int pk;
};

// Mutable per-wave state.  It lives in LDS (not in registers) so that the out-of-line stages below can take the
// context by value and still share it; none of it is touched inside the inner loops.
struct WState {
    uint32_t cur_id;     // stamp of the current grow (id_base + running number)
    int gnum;            // size of the last grow (grow order)
    int has_copy;        // gcopy holds the grow-order list (RegionRadiusReducer reordered lst)
    int tm_pending;      // member masks of evicted tiles stored to HBM since the last fence
    int cache_epoch;     // accept epoch the tile cache was (re)started at; -1: empty
    int members_cached;  // the cache may hold member bits of the last grow
    int ex_upto;         // exact angle sums of the last grow, caught up lazily in list order (myLSD.cpp:545-546)
    double ex_sin, ex_cos;
    Rec rec;             // the rectangle of the region being evaluated
};

struct RCtx {
    int w, h, lane, wave;
    const double* mag;
    const double* deg;
    uint32_t* pw;        // packed pixel words: fp32 angle | usedMap code (shared by the workgroup)
    uint32_t* epochmap;  // accept epoch of code-3 pixels; for growable pixels (code 0 / 2) the LABEL of the certified set they belong to (0: none)
    uint32_t ltag;       // the launch's label tag (see label_make)
    uint32_t* sets;      // this image's certified sets (see "Certified uniform sets" below): [kSetMax + 1] sizes, 0 = dead / unused; null for a helper
    uint32_t* tep;       // per 8x8-pixel tile: epoch + 1 of the latest accepted line with a pixel in it (0: none)
    uint32_t* tmask;     // this wave's member masks of evicted tiles: 4 words per 8x8 tile (grow id, -, 64 member bits)
    uint32_t* spill;
    uint32_t* gcopy;
    float4* meta;        // HBM [mcap]: (unit sum vector, sin of the smallest slack) of the last full test of a list entry, see grow()
    int mcap;
    const double2* sc;   // (sin, cos)(deg)
    int tilesX;
    uint32_t id_base;
    uint32_t id_budget;  // grows a wave may number before it has to clear its member masks (< 2^20: the next run's ids start there)
    double logNT;
    const double* lgamma;
    int lg_count;
    const double* ptab;
    uint32_t* wslist;    // this wave's result slots: [NS][gcap] list entries
    int gcap;
    int llo;             // entries [llo, n) of the current region list are in the LDS ring, entries below in `spill` (grow() keeps g_ctx[wave].llo current)
};
