// region/stats.h -- counters and near-tie accounting: ST_* and sslot, STAT / STATMAX / DSTAT / BSTAT / PSTAT / NOW, the kTie* bounds, TIES_AT and the TS_* sites.  The macros
// add to g_stat[c.wave][] (LDS, declared in lds.h).  Restates nothing of the reference: the bounds are about its libm calls (myLSD.cpp:545-547, :655-665, :973-1004).
enum { ST_GROW = 0, ST_GROWN, ST_NFA, ST_RRR, ST_RRRPASS, ST_SENT, ST_OOB, ST_TREFILL, ST_TOTAL, ST_TGROW, ST_TRECT, ST_TNFA,
       ST_TMARK, ST_SMALLBAIL, ST_WNOSLOT, ST_SEEDS, ST_EXACT, ST_WRING, ST_BATCHES, ST_TTILES, ST_REDO, ST_DISCARD,
       ST_WAIT, ST_SMALLSTEPS, ST_SLOW, ST_TEVAL, ST_TSUMS, ST_TREFINE, ST_TSMALL, ST_TSELECT, ST_TCOMMIT, ST_WNOSEED,
       ST_DEPTHUP, ST_DEPTHDN, ST_DEPTHEND, ST_MINNFA, ST_MINGAP, ST_XEXP, ST_XHELP, ST_TIES, ST_NFASLOW, ST_SETHIT, ST_SETNEW, ST_NFACNT, ST_NFAITER, ST_COUNT,
       ST_GROWANY = ST_COUNT };   // (past the per-word counters: calls of grow_any(), added to bits 8.. of word kStatGrowAnyWord of the record)
static_assert(ST_TOTAL == kStatTotalWord, "lsd_last_region_cycles reads this word");
static_assert(ST_TIES == kStatTiesWord, "lsd_last_sensitivity reads this word");
// STAT: the few per-region counters the parity tests and the bench read (always on).  DSTAT / NOW(): per-batch counters and
// s_memtime stopwatches of the developer build (make STATS=1): they cost ~10 % of the kernel, so the product build has none.
// (every active lane adds the same value to the same word -- no lane-0 branch: a lane-dependent branch whose join block
//  coincides with a join of wave-uniform control flow makes the compiler treat the uniform loop state as divergent)
#ifdef LSD_REGION_STATS
constexpr int kStatSlots = ST_COUNT + 1;
__device__ constexpr int sslot(int i) { return i; }
#else
// the product build keeps the always-on counters only (LDS is the scarce resource of this kernel)
constexpr int kStatSlots = 20;
__device__ constexpr int sslot(int i) {
    return i == ST_GROW ? 0 : i == ST_GROWN ? 1 : i == ST_NFA ? 2 : i == ST_RRR ? 3 : i == ST_RRRPASS ? 4 : i == ST_SENT ? 5 : i == ST_OOB ? 6 :
           i == ST_TOTAL ? 7 : i == ST_SEEDS ? 8 : i == ST_REDO ? 9 : i == ST_DISCARD ? 10 : i == ST_MINNFA ? 12 : i == ST_MINGAP ? 13 : i == ST_XEXP ? 14 : i == ST_XHELP ? 15 : i == ST_SETHIT ? 16 : i == ST_SETNEW ? 17 : i == ST_TIES ? 18 : i == ST_GROWANY ? 19 : 11;
}
#endif
#define STAT(i, v) do { g_stat[c.wave][sslot(i)] += (unsigned long long)(v); } while (0)
// ... and two running maxima (every lane the same value): the smallest |logNFA| RectangleImprover has compared with 0, and the
// smallest non-zero difference between two NFA values it has compared with each other, both kept as kInfBits - bit pattern so
// that the zero-initialised counters work with max (tests/test_parity_gpu.py::test_nfa_decisions_are_far_from_ties)
#define STATMAX(i, v) do { const unsigned long long n_ = (v); if (n_ > g_stat[c.wave][sslot(i)]) g_stat[c.wave][sslot(i)] = n_; } while (0)
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;
// ... and ST_TIES: the number of DECISIONS this image's evaluations took within the noise of the reference's libm (lsd_last_sensitivity,
// include/lsd_hip.h).  The reference's accept / reject decisions hang on glibc's sin / cos / atan2 / exp / log10 / pow, which differ from the
// correctly rounded values computed here by at most one ulp.  A decision "a < b" whose operands are closer than what those ulps can
// move them could come out differently under another libm; each such decision adds one.  0 for an image: every libm within one ulp
// yields the same decisions, hence the same usedMap and lines.  The bounds (upper bounds of the operands' noise, generous: a false
// count costs nothing but information):
//   kTieAng    angles: regDeg = atan2(sum sin, sum cos) of n libm terms -> (n / |V|) 6e-16 + 1e-15 (grow()'s exact test adds n / |V|)
//   kTieFlip   OrientationGetter's comparison of the inertia angle with regDeg (:655-665) and Refiner's wraps
//   kTieRel    the density of a rectangle against denThre, distances against the rectangle's width / Reducer's radius (relative)
//   kTieCoord  a rectangle edge against a pixel row / column (:973-1004), relative: a corner is c + t (dx, dy) with t up to the rectangle's
//              length and (dx, dy) a few ulps of sin / cos off, so it moves by kTieCoord (|c| + length); an edge's height in a column by
//              that times (1 + |slope|) -- the END edges of a rectangle that is almost axis-parallel are steep
// A rectangle whose direction is EXACTLY axis-parallel (min(|dx|, |dy|) < 1e-15: inertiaDeg is 0, pi or +-pi/2 to the last bit, which
// every libm returns alike, and a cosine of 6e-17 moves nothing) has libm-independent coordinates: its exact ties -- edges on pixel
// rows are the rule there -- are not counted.
constexpr double kTieAng = 1e-15, kTieFlip = 1e-13, kTieRel = 1e-12, kTieCoord = 4e-15;
// (developer: -DLSD_TIE_SITES makes the counter a decimal record of WHERE the ties are: three digits per site, see the call sites)
#ifdef LSD_TIE_SITES
__device__ constexpr unsigned long long tie_weight(int site) { unsigned long long w = 1; for (int i = 0; i < site; i++) w *= 1000ull; return w; }
#define TIE_UNIT(site) tie_weight(site)
#else
#define TIE_UNIT(site) 1ull
#endif
#define TIES_AT(site, v) STAT(ST_TIES, (unsigned long long)(v) * TIE_UNIT(site))
enum { TS_GROW = 0, TS_FLIP, TS_DENS, TS_DIST, TS_EDGE, TS_ALIGN, TS_NFA };
__device__ __forceinline__ bool axis_exact(double dx, double dy) { return fmin(fabs(dx), fabs(dy)) < 1e-15; }
#ifdef LSD_REGION_STATS
#define DSTAT(i, v) STAT(i, v)
#define NOW() ((long long)__builtin_amdgcn_s_memtime())
#else
#define DSTAT(i, v) do { } while (0)
#define NOW() 0ll
#endif
// developer experiment (with LSD_REGION_STATS): the time of one grow() batch by segment, in the counters of the per-stage stopwatches
// (rect: entry -> neighbour words read; nfa: -> classified; mark: -> accepted; refine: -> worklist done; sums: between batches)
#ifdef LSD_REGION_BATCHPROF
#define BSTAT(i, v) DSTAT(i, v)
#define PSTAT(i, v) do { } while (0)
#else
#define BSTAT(i, v) do { } while (0)
#define PSTAT(i, v) DSTAT(i, v)
#endif
