// region/eval.h -- one seed's full evaluation (the body of the seed loop, myLSD.cpp:219-272) and what it leaves: refine_tol (Refiner, :804-880), mark_region /
// list_bbox (usedMap marking, :243-248 / :259-265), certify_set (certified uniform sets) and eval_seed.  Reads g_ctx / g_par / g_tol0, writes g_ws[].rec and
// g_eo[]; the lists a speculative result keeps are in the wave's result slots in HBM (RCtx::wslist).  EVAL_CTX / EVAL_GL0 begin and end in eval_seed().
// Refiner, myLSD.cpp:804-880, first half: the re-estimated angle tolerance (:833-855).  The regrow (:857),
// the refit (:866) and the density checks are in the caller's two-pass loop so that grow() and
// rect_convert() are inlined once.
__device__ __noinline__ double refine_tol(int cw_, int sx, int sy, int num, double cenDeg) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int lane = c.lane, w = c.w;
    [[maybe_unused]] const long long t0 = NOW();
    const double rwid = g_ws[c.wave].rec.wid;
    const bool axis0 = axis_exact(g_ws[c.wave].rec.dx, g_ws[c.wave].rec.dy);
    const int wave = __builtin_amdgcn_readfirstlane(c.wave);
    double S = 0;                                 // serial accumulation in list order: lane 0 difSum, 1 squSum
    int ptNum = 0, ties = 0;
    for (int base = 0; base < num; base += 64) {                                   // :839-853
        const int kx = base + lane;
        bool flag = false;
        double degDif = 0;
        if (kx < num) {
            const uint32_t pkx = lget(c, kx);
            const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
            const double ddx = sx - x, ddy = sy - y;
            const double dist = sqrt(ddx * ddx + ddy * ddy);
            if (!axis0 && fabs(dist - rwid) <= kTieRel * (1.0 + rwid)) ties++;    // :845 within the noise of the rectangle's width
            if (dist < rwid) {
                flag = true;
                degDif = c.deg[(size_t)y * w + x] - cenDeg;
                if (fabs(fabs(degDif) - kPi) <= kTieFlip) ties++;                  // :848-851 (two map angles half a turn apart)
                while (degDif <= -kPi) degDif += 2 * kPi;
                while (degDif > kPi) degDif -= 2 * kPi;
            }
        }
        const double sq = degDif * degDif;
        const unsigned long long m = ballot64(flag);
        if (m == 0ull) continue;
        ptNum += __builtin_popcountll(m);
        // (points outside the width contribute +0.0, which leaves a sum that started at +0.0 unchanged to the bit)
        for (int half = 0; half < kStageRounds; half++) {
            const int cnt = min(kStage, num - base - kStage * half);
            if (cnt <= 0) break;
            stage4(wave, lane, half, flag ? degDif : 0.0, flag ? sq : 0.0, 0.0, 0.0);
            S = acc32(wave, lane, cnt, S);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) ties += __shfl_xor(ties, off);
    TIES_AT(TS_DIST, ties);
    const double difSum = rl(S, 0), squSum = rl(S, 1);
    const double meanDif = difSum / (ptNum * 1.0);
    PSTAT(ST_TREFINE, NOW() - t0);
    return 2.0 * sqrt((squSum - 2 * meanDif * difSum) / (ptNum * 1.0) + meanDif * meanDif);   // :855
}

// usedMap marking (:243-248 / :259-265) restricted to the grown pixels; returns their bounding box.
// epoch1 == 0: a rejected region (usedMap = 2); else an accepted line of epoch epoch1 - 1 (usedMap = 1).
struct Box { int x0, y0, x1, y1; };

__device__ __noinline__ Box mark_region(int cw_, uint32_t epoch1, const uint32_t* src, int src_cnt) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int w = c.w;
    [[maybe_unused]] const long long t0 = NOW();
    wg_fence();                                   // (after RegionRadiusReducer: its removals from curMap must have landed)
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    const int cnt = src ? src_cnt : g_ws[c.wave].gnum;
    const bool has_copy = g_ws[c.wave].has_copy != 0;
    const uint32_t cur_id = g_ws[c.wave].cur_id;
    for (int k2 = c.lane; k2 < cnt; k2 += 64) {
        const uint32_t pkx = src ? src[k2] : (has_copy ? c.gcopy[k2] : lget(c, k2));
        const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
        const size_t q = (size_t)y * w + x;
        // curMap == 1 only: a stashed list (src) holds exactly those; the last grow's list is curMap unless RegionRadiusReducer has taken
        // pixels out of it -- then curMap is in tmask (flush_tiles) and the grow-order copy is walked
        if (src || !has_copy || tm_member(c, x, y, cur_id)) {
            const uint32_t old = c.pw[q];
            if (epoch1) {
                if (c.sets) {                              // a banned member ends its certified set (the word holds the set's label until now)
                    const uint32_t lb = label_set(c.ltag, c.epochmap[q]);
                    if (lb) st_l2(&c.sets[lb], 0u);
                }
                c.epochmap[q] = epoch1; c.pw[q] = (old & ~3u) | kPwLine; atomicMax(&c.tep[(y >> 3) * c.tilesX + (x >> 3)], epoch1);
            }
            else c.pw[q] = (old & ~3u) | kPwRejected;
            x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off)); y0 = min(y0, __shfl_xor(y0, off));
        x1 = max(x1, __shfl_xor(x1, off)); y1 = max(y1, __shfl_xor(y1, off));
    }
    PSTAT(ST_TMARK, NOW() - t0);
    Box bx; bx.x0 = x0; bx.y0 = y0; bx.x1 = x1; bx.y1 = y1;
    return bx;
}

// bounding box of `in` and the first num pixels of the region list (of the grow-order copy when from_copy)
__device__ __noinline__ Box list_bbox(int cw_, int num, Box in, bool from_copy) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    int x0 = in.x0, y0 = in.y0, x1 = in.x1, y1 = in.y1;
    for (int k2 = c.lane; k2 < num; k2 += 64) {
        const uint32_t pkx = from_copy ? c.gcopy[k2] : lget(c, k2);
        const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off)); y0 = min(y0, __shfl_xor(y0, off));
        x1 = max(x1, __shfl_xor(x1, off)); y1 = max(y1, __shfl_xor(y1, off));
    }
    Box bx; bx.x0 = x0; bx.y0 = y0; bx.x1 = x1; bx.y1 = y1;
    return bx;
}

// ---------------------------------------------------------------------------------------------
// Certified uniform sets.
//
// A fifth of all pixels the bench batch grows, and nine tenths of its heaviest images', belong to a few sparse structures whose
// pixels all have THE SAME level-line angle, bit for bit (long axis-parallel edges: the seams of the tiled maps, runs of wall),
// grown again from every one of their hundreds of seeds: RegionGrower returns the same ~1 700 pixels, the rectangle around them is
// far too sparse, Refiner re-estimates the tolerance from the pixels near the seed -- all with the seed's own angle, so the new
// tolerance is exactly 0 --, regrows the seed alone and gives up (myLSD.cpp:833-861): nothing is marked, and the next seed of the
// structure starts over (the reference does exactly that).  For such a set S the whole evaluation of ANY seed in S is known without
// growing anything, provided
//   (1) every pixel of S has the angle theta (fp64 equality) and is growable (not banned);
//   (2) every growable pixel next to S that is not in S is further than tol + 1e-5 from theta (circular distance; for tol < pi/2 the
//       reference's test :540-543 IS the circular distance; the 1e-5 covers the packed fp32 angle the check reads, 1.2e-6);
//   (3) S is 8-connected (it is: it was grown as one region);
//   (4) the rectangle of S is sparse by a margin: density < denThre (1 - 1e-3).
// (1)-(3): whatever seed B in S the reference starts from, regDeg is theta at every step (the sum of equal unit vectors has their
// direction; atan2's rounding is many orders below the 1e-5), every member passes its test the first time it comes up and every
// other growable neighbour fails every time: RegionGrower returns S, |S| >= regThre.  (4): the density of the rectangle depends on
// the list order only through the rounding of its sums (relative 1e-10 for 65 535 pixels), so it is below denThre for every seed.
// Refiner then sees angle differences of exactly 0 (:839-853: degDif = theta - theta), tol = 2 sqrt(0) = 0, regrows the seed alone
// (:857, `0 < 0` never holds) and fails at :861.  Outcome: no marks, first region |S| pixels, final region 1 pixel.
//
// Mechanics.  epochmap[] is free for growable pixels (it holds the accept epoch of banned ones): there it carries the LABEL of the
// pixel's set, tagged with the launch's run number (label_make: what earlier launches left in the buffer is no label of this one).  An evaluation that went exactly this way (EvalOut.cert) offers its first list: certify_set() checks
// (1) and labels the members under the cursor lock -- the lock commits hold, so no ban can slip between check and label --, checks
// (2) and publishes the set's size in sets[label].  A line that bans a member clears sets[label] (mark_region: the label is still in
// the word it overwrites with the epoch).  Invariant: every member of a live set carries its label (a new set that takes over a
// labelled pixel ends the older set).  eval_seed() looks at its seed's label first; a live set answers at once (EvalOut.setid).  The
// result waits in the ring as R_SETL and is valid at its turn iff the set is still alive -- alive means no member was ever banned,
// which is exactly "no member banned since the snapshot" for a result that has ALL of S as its list.  Wavefronts that help another
// image neither use nor found sets (labels and table are read through this CU's caches).
// ---------------------------------------------------------------------------------------------
__device__ __noinline__ int certify_set(int cw_, uint32_t pp_, int slot_, int n_, int* lock_, int* nsets_) {
    const int wave = uni(cw_);
    const int lane = (int)(threadIdx.x & 63);
    const RCtx c = g_ctx[wave];
    const int w = uni(c.w), h = uni(c.h), n = uni(n_);
    const uint32_t pp = (uint32_t)uni((int)pp_);
    const uint32_t* const list = c.wslist + (size_t)uni(slot_) * uni(c.gcap);     // the first grow's list, kept for the cursor's validation
    uint32_t* const sets = c.sets;
    {   // the structure has its set already (another wavefront's evaluation of a neighbouring seed got here first): nothing to found
        const uint32_t lb0 = label_set(c.ltag, (uint32_t)uni((int)c.epochmap[pp]));
        if (lb0 && (uint32_t)uni((int)ld_l2(&sets[lb0])) != 0u) return 0;
    }
    int got = 0;
    if (lane == 0) got = atomicCAS(lock_, 0, 1) == 0 ? 1 : 0;                     // (busy: the next seed of the structure will offer again)
    if (!uni(got)) return 0;
    {   // (again under the lock: labels and table only change under it)
        const uint32_t lb0 = label_set(c.ltag, (uint32_t)uni((int)c.epochmap[pp]));
        if (lb0 && (uint32_t)uni((int)ld_l2(&sets[lb0])) != 0u) {
            if (lane == 0) __hip_atomic_store(lock_, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            return 0;
        }
    }
    int id = 0;
    if (lane == 0) { id = *nsets_ + 1; if (id <= kSetMax) *nsets_ = id; }
    id = uni(id);
    bool bad = id > kSetMax;
    if (!bad) {
        // (1) + labels, under the lock
        const double theta = c.deg[pp];
        for (int base = 0; base < n; base += 64) {
            const int k2 = base + lane;
            if (k2 < n) {
                const uint32_t pk = list[k2];
                const size_t q = (size_t)(pk >> 16) * w + (pk & 0xffffu);
                const uint32_t code = c.pw[q] & 3u;
                if (code != kPwFree && code != kPwRejected) bad = true;              // banned meanwhile (its word holds the line's epoch: hands off)
                else {
                    if (c.deg[q] != theta) bad = true;
                    const uint32_t lb = label_set(c.ltag, c.epochmap[q]);
                    if (lb && lb != (uint32_t)id) st_l2(&sets[lb], 0u);   // an older set loses a pixel: it ends
                    c.epochmap[q] = label_make(c.ltag, (uint32_t)id);
                }
            }
        }
        bad = ballot64(bad) != 0ull;
        if (lane == 0) st_l2(&sets[id], bad ? 0u : ((uint32_t)n | kSetPending));
        wg_fence();
    }
    if (lane == 0) __hip_atomic_store(lock_, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (bad) return 0;
    // (2) the growable neighbours outside S, without the lock: a pixel that fails now fails for good (bans only grow, angles never change)
    const float thf = __uint_as_float(c.pw[pp] & ~3u);
    const float lim = (float)g_tol0[0] + 1e-5f;
    const int e = lane >> 3, k8 = lane & 7, kk = k8 + (k8 >= 4);
    const int ox = kk % 3 - 1, oy = kk / 3 - 1;
    for (int base = 0; base < n; base += 8) {
        const int k2 = base + e;
        if (k2 < n) {
            const uint32_t pk = list[k2];
            const int nx = (int)(pk & 0xffffu) + ox, ny = (int)(pk >> 16) + oy;
            if (((unsigned)nx < (unsigned)w) & ((unsigned)ny < (unsigned)h)) {
                const size_t q = (size_t)ny * w + nx;
                const uint32_t wq = c.pw[q], lb = label_set(c.ltag, c.epochmap[q]);
                const uint32_t code = wq & 3u;
                if ((code == kPwFree || code == kPwRejected) && lb != (uint32_t)id) {
                    float d = fabsf(__uint_as_float(wq & ~3u) - thf);
                    if (d > (float)kPi) d = 2.0f * (float)kPi - d;
                    if (d < lim) bad = true;
                }
            }
        }
    }
    bad = ballot64(bad) != 0ull;
    int alive = 0;
    if (lane == 0) {
        if (bad) st_l2(&sets[id], 0u);
        else alive = atomicCAS(&sets[id], (uint32_t)n | kSetPending, (uint32_t)n) == ((uint32_t)n | kSetPending) ? 1 : 0;   // (0 meanwhile: a member was banned)
    }
    return uni(alive) ? id : 0;
}

// One seed's evaluation, RegionGrower ... RectangleImprover (:225-240), with all 64 lanes of the wave; pp = the seed's pixel.
// A speculative evaluation (spec != 0) also leaves in result slot `slot` what the commit at the cursor will need: the first
// grow's list and Refiner's regrow (their pixels decide whether the result is still valid at its turn), and the pixels to mark.
// The outcome goes to g_eo[wave] (all lanes store the same values), the rectangle stays in g_ws[wave].rec.
__device__ __noinline__ void eval_seed(int cw_, uint32_t pp_, int spec_, int slot_) {
    // What lives across this function's calls is wave-uniform and kept in scalar registers (uni()): values in VECTOR registers that
    // survive a call have to sit in callee-saved ones, which this function must then save and restore through scratch memory for ITS
    // caller -- 59 registers per evaluation before this was done, the largest single writer of the stage's HBM traffic.  The wave's
    // context is read from LDS where it is needed instead of being carried along.
    const int wave = uni(cw_);
    const int lane = (int)(threadIdx.x & 63);
    const int w = uni(g_ctx[wave].w), gcap = uni(g_ctx[wave].gcap);
    const uint32_t pp = (uint32_t)uni((int)pp_);
    const bool spec = uni(spec_) != 0;
    const int slot = uni(slot_);
    const double p_degThre = uni(g_par[0]), p_regThre = uni(g_par[1]), p_aliPro = uni(g_par[2]), p_denThre = uni(g_par[3]);
    const int sx = uni((int)(pp % (uint32_t)w)), sy = uni((int)(pp / (uint32_t)w));
    EvalOut& eo = g_eo[wave];
#define EVAL_CTX() RCtx c = g_ctx[wave]; c.lane = lane
#define EVAL_GL0() (g_ctx[wave].wslist + (size_t)slot * gcap)

    int outcome = 0, num = 0, num0 = 0, rec_pk = 0;
    double logNFA = 0;
    const bool skip = uni((int)(g_ctx[wave].pw[pp] & 3u)) != 0;   // monotone: once used, always used (:222)
    eo.setid = 0; eo.cert = 0;
    if (!skip && g_ctx[wave].sets) {
        // a seed of a live certified set: the evaluation is known (see "Certified uniform sets")
        const uint32_t lb = label_set((uint32_t)uni((int)g_ctx[wave].ltag), (uint32_t)uni((int)g_ctx[wave].epochmap[pp]));
        if (lb) {
            const uint32_t ns = (uint32_t)uni((int)ld_l2(&g_ctx[wave].sets[lb]));
            if (ns >= (uint32_t)kSetMinPixels && ns < kSetPending && (double)ns >= p_regThre) {
                RCtx c = g_ctx[wave]; c.lane = lane;
                STAT(ST_GROW, 2); STAT(ST_GROWN, ns + 1u);             // (RegionGrower's two calls of the reference, as the work counters count them)
                STAT(ST_SETHIT, 1);
                eo.skip = 0; eo.outcome = 1; eo.num = 1; eo.num0 = (int)ns; eo.rec_pk = 0; eo.logNFA = 0;
                eo.redo = 0; eo.precise = 0; eo.n1 = 0; eo.n2 = 0; eo.m_off = 0; eo.mcnt = 1;
                eo.x0 = 0; eo.y0 = 0; eo.x1 = -1; eo.y1 = -1;
                eo.setid = (int)lb;
                return;
            }
        }
    }
    int fx0 = 0x7fffffff, fy0 = 0x7fffffff, fx1 = -1, fy1 = -1;   // box of a first grow that refine() replaced
    bool sparse_by_margin = false, tol_zero = false;
    // list slot of a speculative evaluation: [first grow (n1)][Refiner's regrow (n2)][pixels to mark, if not one of those]
    int n1 = -1;                                       // -1: the lists are not kept (validation by bounding box only)
    bool regrown = false;
    if (!skip) {
        // RegionGrower -> RectangleConverter -> Refiner (:225-238) as a two-pass loop: pass 0 grows with the
        // global tolerance, pass 1 (only when the rectangle is too sparse, :829) regrows with the tolerance
        // re-estimated by Refiner (:833-857).
        const double seedDeg = uni(g_ctx[wave].deg[pp]);
        double tol = p_degThre, regdeg = seedDeg;
        bool done = false;
        for (int pass = 0; pass < 2 && !done; pass++) {
            // (by tolerance class, region/grow.h: tol is wave-uniform, a NaN goes with the large ones)
            num = uni(uni((int)(tol < 1.5)) ? grow(wave, sx, sy, seedDeg, tol) : grow_any(wave, sx, sy, seedDeg, tol));   // :225 / :857
            if (pass == 0 && spec && num <= gcap) {                // keep the first list for the validation at the cursor
                EVAL_CTX();
                uint32_t* const gl0 = EVAL_GL0();
                for (int k2 = lane; k2 < num; k2 += 64) gl0[k2] = lget(c, k2);
                n1 = num;
            }
            if (pass == 1) regrown = true;
            if (pass == 0) {
                num0 = num;
                if (num < p_regThre) { done = true; break; }                      // :228 (not marked, Q5)
            } else if (num < 2) { outcome = 1; done = true; break; }              // :861
            if (num > 1) { exact_sums(wave, num); regdeg = uni(atan2_g(g_ws[wave].ex_sin, g_ws[wave].ex_cos)); }   // reg.deg (:547, :581)
            else regdeg = seedDeg;
            rect_convert(wave, num, regdeg, p_aliPro, 0, p_degThre);                   // :232 / :866 (p, prec still the defaults)
            const double den = uni(rec_density(num, g_ws[wave].rec));
            if (fabs(den - p_denThre) <= kTieRel * p_denThre && !axis_exact(g_ws[wave].rec.dx, g_ws[wave].rec.dy))     // :829 / :869 within the libm's noise
                g_stat[wave][sslot(ST_TIES)] += TIE_UNIT(TS_DENS);
            if (pass == 0) {
                if (den >= p_denThre) break;                                      // :829 dense enough
                sparse_by_margin = den < p_denThre * (1.0 - 1e-3);
                if (spec) {                                                       // the regrow replaces this list
                    Box fb; fb.x0 = fx0; fb.y0 = fy0; fb.x1 = fx1; fb.y1 = fy1;
                    fb = list_bbox(wave, num, fb, false);
                    fx0 = uni(fb.x0); fy0 = uni(fb.y0); fx1 = uni(fb.x1); fy1 = uni(fb.y1);
                }
                tol = uni(refine_tol(wave, sx, sy, num, seedDeg));                     // :833-855
                tol_zero = tol == 0.0;
            } else if (den < p_denThre) {                                         // :869-877
                const int r = uni(radius_reduce(wave, sx, sy, num, regdeg, p_denThre));   // (lst reordered: gcopy holds the grow-order list)
                if (r < 0) { num = -r - 1; outcome = 1; done = true; }
                else num = r;
            }
        }
        if (!done) {
            logNFA = uni(improve(wave));                                               // :240
            outcome = logNFA <= 0 ? 2 : 3;                                        // :242
            rec_pk = uni(g_ws[wave].rec.pk);
        }
    }
    eo.skip = skip ? 1 : 0; eo.outcome = outcome; eo.num = num; eo.num0 = num0; eo.rec_pk = rec_pk; eo.logNFA = logNFA;
    eo.redo = 0; eo.precise = 0; eo.n1 = 0; eo.n2 = 0; eo.m_off = 0; eo.mcnt = num;
    // the way every seed of a uniform set goes: a sparse first region, a re-estimated tolerance of exactly 0, the seed alone, given up
    eo.cert = (spec && !skip && outcome == 1 && regrown && num == 1 && sparse_by_margin && tol_zero && n1 == num0 && num0 >= kSetMinPixels &&
               num0 <= 65535 && p_degThre < 1.5 && g_ctx[wave].sets != nullptr) ? 1 : 0;
    if (!spec || skip) return;

    const int gnum = uni(g_ws[wave].gnum);             // size of the last grow (grow order)
    const bool has_copy = uni(g_ws[wave].has_copy) != 0;
    // box of the pixels of this evaluation's grown lists
    {                                                  // (RegionRadiusReducer reordered/shrunk lst: the grow-order copy then)
        Box fb; fb.x0 = fx0; fb.y0 = fy0; fb.x1 = fx1; fb.y1 = fy1;
        fb = list_bbox(wave, gnum, fb, has_copy);
        eo.x0 = fb.x0; eo.y0 = fb.y0; eo.x1 = fb.x1; eo.y1 = fb.y1;
    }
    EVAL_CTX();
    uint32_t* const gl0 = EVAL_GL0();
    const unsigned long long ltm = (1ull << lane) - 1ull;
    bool precise = n1 >= 0;
    int n2 = 0;
    if (regrown) {                                     // keep Refiner's regrow (in grow order, before any reduction) behind the first list
        if (precise && n1 + gnum <= gcap) {
            for (int k2 = lane; k2 < gnum; k2 += 64) gl0[n1 + k2] = has_copy ? c.gcopy[k2] : lget(c, k2);
            n2 = gnum;
        } else precise = false;
    }
    if (n1 > 32767 || n2 > 32767) precise = false;     // (the sizes travel in 15-bit fields)
    eo.precise = precise ? 1 : 0; eo.n1 = n1; eo.n2 = n2;
    if (outcome <= 1) return;                          // nothing to mark
    // the pixels to mark
    int m_off = 0, mcnt = num;                         // not regrown: the first list is exactly the region
    bool redo = false;
    if (!regrown) {
        if (!precise) redo = true;                     // (larger than a list slot) evaluate again at the cursor
    } else if (precise && !has_copy) { m_off = n1; mcnt = n2; }            // the regrow as it is
    else {
        m_off = precise ? n1 + n2 : 0;
        if (m_off + gnum > gcap) { precise = false; m_off = 0; }
        if (gnum > gcap) redo = true;
        else {
            wg_fence();                                // (RegionRadiusReducer's removals from curMap must have landed)
            const uint32_t cur_id = g_ws[wave].cur_id;
            mcnt = 0;
            for (int base = 0; base < gnum; base += 64) {
                const int k2 = base + lane;
                uint32_t pkx = 0;
                bool keep = false;
                if (k2 < gnum) {
                    pkx = has_copy ? c.gcopy[k2] : lget(c, k2);
                    keep = !has_copy || tm_member(c, (int)(pkx & 0xffffu), (int)(pkx >> 16), cur_id);   // curMap == 1 only
                }
                const unsigned long long km = ballot64(keep);
                if (keep) gl0[m_off + mcnt + __builtin_popcountll(km & ltm)] = pkx;
                mcnt += __builtin_popcountll(km);
            }
        }
    }
    eo.precise = precise ? 1 : 0; eo.m_off = m_off; eo.mcnt = mcnt; eo.redo = redo ? 1 : 0;
#undef EVAL_CTX
#undef EVAL_GL0
}
