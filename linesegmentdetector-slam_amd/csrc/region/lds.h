// region/lds.h -- the stage's namespace-scope LDS: the per-wave arena and its three views (G_LST list ring, G_WL worklist, G_TW tile cache), g_ttag,
// g_stat, g_ws, g_ctx, g_tol0, g_acc, g_eo (EvalOut), g_par; and stage4 / acc32, the serial sums over g_acc that keep the reference's left-to-right
// fp64 additions (myLSD.cpp:545-546, :608-613, :637-643, :839-853).
// Per-wave LDS storage.  Declared at namespace scope (not inside the kernel) so that the out-of-line stages address it
// as LDS (ds_ instructions) instead of through generic pointers carried in the context (flat_ instructions).
// One arena of 32-bit words per wave, used in two ways.  A full evaluation: [list ring, LCAP words (packed y<<16 | x)][the sweep
// worklist, WCAP 16-bit entries + a dummy slot for predicated stores: list indices of the entries that still have a growable
// neighbour; the next sweep's worklist is written IN PLACE behind the read cursor][tile cache, NT x 64 words: (fp32 angle & ~3) |
// member << 1 | banned].  The small-region grower (seed loop): [eight windows of 16 x kWinRows pixels][eight lists of SCAP entries] from the
// start of the arena -- nothing of a full evaluation survives it (tw_small in the seed loop).
constexpr int SCAP = 16;                  // list entries of a small-region group
constexpr int kSmallWords = 8 * kWinWords + 8 * SCAP;
constexpr int WLW = ((kSmallWords - LCAP - NT * 64 >= 256 ? kSmallWords - LCAP - NT * 64 : 256) + 3) & ~3; // words of the worklist (16-byte multiple: windows and tiles are written as uint4)
constexpr int WCAP = 2 * WLW - 2;                            // its entries; [WCAP]: the dummy slot
constexpr int kTwOff = LCAP + WLW;
constexpr int kArenaWords = kTwOff + NT * 64 > kSmallWords ? kTwOff + NT * 64 : kSmallWords;
constexpr int kMvCap = kArenaWords - LCAP - 1;               // RegionRadiusReducer's scratch: worklist + tile cache (+ a dummy slot)
static_assert(WLW >= 192, "the NFA's column scan keeps 3 x 64 ints in the worklist's place");
// both layouts fit the arena; a neighbour one row or column outside a window is still read (and ignored), from inside the arena
static_assert(kSmallWords <= kArenaWords && kTwOff + NT * 64 <= kArenaWords && 7 * kWinWords + 255 < kArenaWords, "the small grower's and the full evaluation's layouts both fit the arena");
__shared__ __attribute__((aligned(16))) uint32_t g_arena[NW][kArenaWords];
#define G_ARENA(w) (&g_arena[w][0])
#define G_LST(w) (G_ARENA(w))
#define G_WL(w) (reinterpret_cast<uint16_t*>(G_ARENA(w) + LCAP))
#define G_TW(w) (G_ARENA(w) + kTwOff)
__shared__ int g_ttag[NW][NT];
__shared__ unsigned long long g_stat[NW][kStatSlots];      // per-wave counters (see ST_* above); kept out of registers
__shared__ WState g_ws[NW];
__shared__ RCtx g_ctx[NW];                                // the wave's context: the out-of-line stages get the wave number and read it here
                                                          // (a struct passed by value travels through scratch memory at every call)
__shared__ double g_tol0[3];                              // the global tolerance (degThre) with its sine and cosine: every first grow uses it
__shared__ double g_acc[NW][kStage * 4];                  // staging of the serial (bit-exact) sums: kStage list elements x up to 4 terms
// what eval_seed() leaves for its caller (the rectangle itself stays in g_ws[wave].rec)
struct EvalOut {
    int skip, outcome, num, num0, rec_pk;
    int x0, y0, x1, y1;      // box of the pixels of the grown lists (speculative evaluations only)
    int n1, n2, precise;     // sizes of the first grow and of Refiner's regrow kept in the slot (precise == 0: not kept)
    int m_off, mcnt, redo;   // where the pixels to mark sit in the slot; redo: the result does not fit a slot
    int setid;               // != 0: the result was taken from certified set `setid` without growing anything (outcome 1)
    int cert;                // 1: this evaluation went the way every seed of a uniform set goes (see certify_set): its first list may found a set
    double logNFA;
};
__shared__ EvalOut g_eo[NW];
__shared__ double g_par[4];                               // degThre, regThre, aliPro, denThre of the launch (Geom)

// The reference's sums over a region (moments, angle sums, Refiner's statistics) are plain left-to-right fp64 additions, and
// their rounding decides accept/reject ties, so they are added in exactly that order: the lanes compute the terms of kStage list
// elements at a time and stage them in LDS, then lane j (j < 4) adds term j of the elements one after the other.  (One
// ds_read + one v_add per element and sum, all sums at once, instead of broadcasting every term to every lane.)
constexpr int kStageRounds = 64 / kStage;   // rounds that take the 64 elements of a wave's chunk through the staging
__device__ __forceinline__ void stage4(int wave, int lane, int part, double t0, double t1, double t2, double t3) {
    if (lane / kStage == part) {
        double* q = &g_acc[wave][(lane % kStage) * 4];
        q[0] = t0; q[1] = t1; q[2] = t2; q[3] = t3;
    }
}
__device__ __forceinline__ double acc32(int wave, int lane, int cnt, double S) {   // cnt (wave-uniform) <= kStage staged elements
    const double* q = &g_acc[wave][lane & 3];
    int e = 0;
    for (; e + 8 <= cnt; e += 8) {
        S += q[(e + 0) * 4]; S += q[(e + 1) * 4]; S += q[(e + 2) * 4]; S += q[(e + 3) * 4];
        S += q[(e + 4) * 4]; S += q[(e + 5) * 4]; S += q[(e + 6) * 4]; S += q[(e + 7) * 4];
    }
    for (; e < cnt; e++) S += q[e * 4];
    return S;
}
