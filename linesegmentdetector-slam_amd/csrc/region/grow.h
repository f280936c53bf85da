// region/grow.h -- RegionGrower (myLSD.cpp:491-590) with all 64 lanes of a wave: exact_sums (the angle sums, :545-546), the helpers of the fp32 estimate
// (inv_ub, kEpsU, fast_sincos) and grow() / grow_any().  Touches the whole arena (list ring G_LST, worklist G_WL, tile cache through tiles.h), g_ws, g_ctx[].llo,
// g_tol0 and g_acc; list entries that left the ring and the slack records are in HBM (RCtx::spill, RCtx::meta).  GROW_ESTIMATE begins and ends in grow().
// ---------------------------------------------------------------------------------------------
// The exact angle sums of the current region (sinDeg, cosDeg of RegionGrower, :545-546) over the list prefix
// [0, n): the reference adds cos/sin(deg) of every accepted pixel in the order of acceptance, which is the list
// order, so the sums can be caught up at any time from the list and the (sin, cos) map K2 wrote.
// ---------------------------------------------------------------------------------------------
// (out of line, like every per-region stage below: each gets the register file to itself, and the seed loop keeps only
//  what it needs across the calls; the context travels by value, the mutable state sits in LDS)
__device__ __noinline__ void exact_sums(int cw_, int n_) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane(c.wave), n = __builtin_amdgcn_readfirstlane(n_);
    const int from = __builtin_amdgcn_readfirstlane(g_ws[wave].ex_upto);
    if (from >= n) return;
    [[maybe_unused]] const long long t0 = NOW();
    const int lane = c.lane, w = c.w;
    double S = lane == 0 ? g_ws[wave].ex_cos : g_ws[wave].ex_sin;      // lane 0: cosDeg, lane 1: sinDeg (:545-546)
    for (int base = from; base < n; base += 64) {
        const int kx = base + lane;
        double vs = 0, vc = 0;
        if (kx < n) {
            const uint32_t pk = lget(c, kx);
            const double2 v = c.sc[(size_t)(pk >> 16) * w + (pk & 0xffffu)];
            vs = v.x; vc = v.y;
        }
        for (int half = 0; half < kStageRounds; half++) {
            const int cnt = min(kStage, n - base - kStage * half);
            if (cnt <= 0) break;
            stage4(wave, lane, half, vc, vs, 0.0, 0.0);
            S = acc32(wave, lane, cnt, S);
        }
    }
    if (lane == 0) { g_ws[wave].ex_cos = S; g_ws[wave].ex_upto = n; }
    if (lane == 1) g_ws[wave].ex_sin = S;
    PSTAT(ST_TSUMS, NOW() - t0);
}

// ---------------------------------------------------------------------------------------------
// RegionGrower, myLSD.cpp:491-590.  Leaves the region in c.lst (grow order) and returns its size; the angle
// sums are available through exact_sums() (the caller needs them only for regions that go on to the rectangle).
//
// The reference tests every candidate against regDeg = atan2(sinDeg, cosDeg) recomputed after each accepted
// pixel (:545-547), in list order / row-major neighbour order.  For tol < pi/2 "|regDeg - deg| (wrapped) < tol"
// is the circular distance between the candidate's direction u and the direction of the sum vector V, i.e.
// u.V > cos(tol) |V|.  A batch of 8 frontier pixels x 8 neighbours is classified at once in that form with fp32
// ESTIMATES of u (hardware sin/cos of the packed fp32 angle) and V (their running sum), and a rigorous margin:
//   eps_c  error of the estimated cosine: |u - u_true| <= kEpsU per vector, so V is off by <= n kEpsU
//   delta  largest turn of V while the up-to-m winners of this batch are accepted: each accepted unit vector lies
//          within tol of the current sum of norm L, so it turns it by at most sin(tol)/L
//   * cos > cos(tol) + delta sin(tol) + eps_c      : passes whatever happens earlier in the batch -> accepted in bulk
//   * cos < cos(tol) - delta (sin(tol)+delta) - eps_c : fails whatever happens                    -> ignored
//   * otherwise the batch is resolved pixel by pixel in reference order against the then-current estimate, and
//     against the correctly rounded angle of the exact sums when still too close to call.
// Every accept/reject decision is therefore the one the exact angle would give; the exact sums are accumulated in
// reference order (exact_sums()).  Larger tolerances (Refiner may ask for any) take the pixel-by-pixel path with the
// reference's own wrapped-difference test.
// Sweeps after the first revisit only entries that still had a non-member, non-banned neighbour
// (membership and bans only grow during one call, so the others cannot accept anything).
// ---------------------------------------------------------------------------------------------

// an upper bound of 1 / v for v >= 0.9 (v_rcp_f32 is good to 1 ulp; the margins it feeds are themselves upper bounds)
__device__ __forceinline__ float inv_ub(float v) { return __builtin_amdgcn_rcpf(v) * 1.000001f; }

constexpr float kEpsU = 6e-6f;     // >= |(cos, sin) estimate - exact| per accepted pixel: 2-bit truncation of the fp32 angle (1e-6) + v_sin/v_cos_f32
                                   //    (together <= 3e-6: tests/test_parity_gpu.py::test_fast_sincos_error_bound) + the fp32 partial sums of
                                   //    a batch (<= 64 terms: <= 2^-24 * 32 = 1.9e-6 per term); the running sums themselves are fp64
constexpr float kInv2Pi = 0.15915494309189535f;

__device__ __forceinline__ void fast_sincos(float a, float& s, float& co) {   // hardware sin/cos take revolutions
    const float r = a * kInv2Pi;
    s = __builtin_amdgcn_sinf(r);
    co = __builtin_amdgcn_cosf(r);
}

// Written once, compiled per TOLERANCE CLASS (the callers are grow() and grow_any() below): kTolSmall -- tol < 1.5, every first grow at the
// default angThre and nearly all of Refiner's regrows: the circular-distance form alone; else -- any other tolerance, NaN included: the
// pixel-by-pixel form with the reference's wrapped difference (fp64 atan2) alone.  Every decision is taken by the same expressions as when
// one function held both; each class lacks only the code that cannot run for it.  Under the 4-wave build's 128 registers that is what
// matters: a function saves its callee-saved registers at every call whether or not the path that needs them runs, and without the
// any-tolerance path grow() puts away 22 registers instead of 52 ("grow() by tolerance class").
template <bool kTolSmall>
__device__ __forceinline__ int grow_body(int cw_, int sx_, int sy_, double regDeg0_, double tol_) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int lane = c.lane;
    const double regDeg0 = uni(regDeg0_), tol = uni(tol_);
    const int w = uni(c.w), h = uni(c.h), wave = uni(c.wave), mcap = uni(c.mcap);
    const int sx = uni(sx_), sy = uni(sy_);
    AS1 nf4* const meta = (AS1 nf4*)uglobal(c.meta);
    c.w = w; c.h = h; c.wave = wave;                         // (what the helpers below read)
    [[maybe_unused]] const long long t0 = NOW();
    // curMap of the previous grow: drop its member flags from the cache (:519 starts from zeros)
    if (uni(g_ws[wave].members_cached)) {
        const int gprev = uni(g_ws[wave].gnum);
        if (uni(g_ws[wave].has_copy) || gprev > 4 * LCAP) invalidate_tiles(c);
        else {
            for (int k2 = lane; k2 < gprev; k2 += 64) {
                const uint32_t pk = lget(c, k2);
                const int x = (int)(pk & 0xffffu), y = (int)(pk >> 16);
                const int slot = tile_slot(x >> 3, y >> 3);
                if (g_ttag[wave][slot] == tile_key(x >> 3, y >> 3)) G_TW(wave)[slot * 64 + ((y & 7) << 3) + (x & 7)] &= ~2u;
            }
        }
    }
    uint32_t id = (uint32_t)uni((int)g_ws[wave].cur_id);
    if ((id - (uint32_t)uni((int)c.id_base)) >= (uint32_t)uni((int)c.id_budget)) {                      // the run's 2^20 stamp ids are used up: start over on clean stamps
        const uint32_t tmw = 4u * (uint32_t)(c.tilesX * ((h + 7) >> 3));
        for (uint32_t q = lane; q < tmw; q += 64) c.tmask[q] = 0u;
        wg_fence();
        id = c.id_base;
    }
    id = (uint32_t)uni((int)id + 1);                         // fresh curMap (:519)
    if (lane == 0) {
        WState& ws = g_ws[wave];
        ws.cur_id = id; ws.members_cached = 1; ws.has_copy = 0; ws.ex_upto = 0; ws.ex_sin = 0.0; ws.ex_cos = 0.0;
        g_ctx[wave].llo = 0;                                 // the new list starts inside the ring
    }
    c.llo = 0;
    AS1 uint32_t* const spill = uglobal(c.spill);
    ensure_tiles(c, lane == 0, sx, sy);
    double Ce, Se;                                           // estimated sum vector (fp64 accumulation of the fp32 unit vectors)
    {
        const int slot = tile_slot(sx >> 3, sy >> 3), ti = ((sy & 7) << 3) | (sx & 7);
        const uint32_t sw = G_TW(wave)[slot * 64 + ti];
        float s0, c0;
        fast_sincos(__uint_as_float(sw & ~3u), s0, c0);
        Ce = (double)c0; Se = (double)s0;
        if (lane == 0) {
            G_LST(wave)[0] = pack_xy(sx, sy);
            G_TW(wave)[slot * 64 + ti] = sw | 2u;            // :520
        }
    }
    int n = 1;
    bool wt = false;                                         // the list has outgrown the ring: entries are also written through to `spill`
    if (!kTolSmall && !(tol == tol)) {                       // NaN tolerance (Refiner, :855): no test ever passes (NaN < 1.5 is false: never in class 1)
        if (lane == 0) g_ws[wave].gnum = 1;
        STAT(ST_GROW, 1); STAT(ST_GROWN, 1); STAT(ST_GROWANY, 1);
        return 1;
    }
    constexpr bool tol_small = kTolSmall;                    // (tol < 1.5: eval_seed() chooses) the circular-distance form applies, and accepted vectors never shorten the sum
    const float turn = (float)(tol < 1.1 ? tol : 1.1) * 1.0032f;   // >= sin(tol) resp. the asin(1/L)*L bound, x (|V| estimate / its lower bound)
    const float tolf_lo = (float)tol * 0.9999999f;           // <= tol
    float cos_tol, sin_tol;
    {
        double st, ct;
        if (tol == g_tol0[0]) { st = g_tol0[1]; ct = g_tol0[2]; }           // (wave-uniform)
        else sincos_g(tol_small ? tol : 1.0, st, ct);
        cos_tol = (float)ct; sin_tol = (float)st * 1.0000002f + 1e-7f;      // sin_tol >= sin(tol)
    }
    const int e = lane >> 3, k = lane & 7;
    const int kk = k + (k >= 4);                             // 3x3 neighbourhood, row-major, centre skipped (:533-534)
    const int ox = kk % 3 - 1, oy = kk / 3 - 1;
    int wl_cnt = 0;                                          // entries of this sweep's worklist (sweep >= 2)
    bool filter = true;                                      // false once the list outgrew the worklist
    // Re-sweeps: an entry whose remaining candidates all failed by more than the sum vector has turned since cannot
    // accept anything now either (membership and bans only grow); it is carried over to the next worklist without
    // touching its neighbourhood.  meta[entry] = (unit sum vector its candidates were compared with, sine of the
    // smallest "distance - tol" among the candidates left), checked 64 entries at a time.
    unsigned long long flt_need = 0;                         // chunk [flt_base, flt_base + 64) of the worklist: entries to test in full
    int flt_base = 0;
    bool flt_valid = false;
    int nxt_cnt = 0;                                         // entries of the next sweep's worklist
    [[maybe_unused]] long long bt_last = NOW();
    // One batch: up to 8 list entries (cnt of them, entry e of the batch = list index eidx in its 8 lanes) x 8 neighbours.
    // Returns the number of entries it dealt with (1 instead of cnt when their tiles collide in the cache).
    auto batch = [&](int cnt, const int eidx, const bool direct, const float Cf, const float Sf, const float rV, const float Vn,
                     const float nrat) -> int {
        [[maybe_unused]] const long long bt0 = NOW();
        BSTAT(ST_TSUMS, bt0 - bt_last);
        bool valid = e < cnt;
        // (entries past n: harmless garbage, masked by valid.)  The LDS part of the list is read unconditionally and the HBM part
        // in a block of its own that also waits for it: a load whose register is still pending at the join would make the
        // compiler put an s_waitcnt vmcnt(0) in front of every batch, and that waits for the stamp stores of the batch before.
        uint32_t pk = G_LST(wave)[eidx & LMASK];
        if (!direct) {                                       // entries that have left the ring (wave-uniform: only a list longer than the ring has any)
            const int lo = wt ? n - LCAP : 0;
            if (ballot64(valid & (eidx < lo))) {
                uint32_t t = pk;
                if (valid & (eidx < lo)) t = spill[(uint32_t)eidx];
                asm volatile("; spilled list entry %0" :: "v"(t));
                pk = t;
            }
        }
        const int nx = (int)(pk & 0xffffu) + ox, ny = (int)(pk >> 16) + oy;
        bool inb = valid & ((unsigned)nx < (unsigned)w) & ((unsigned)ny < (unsigned)h);   // :536 (plain &: no short-circuit branches)
        const int tx = nx >> 3, ty = ny >> 3;
        const int slot = tile_slot(tx, ty);
        const int cell = (slot << 6) | ((ny & 7) << 3) | (nx & 7);        // (in range even for !inb lanes)
        uint32_t word_r = G_TW(wave)[cell];
        int tagv = g_ttag[wave][slot];
        // (both reads in flight before the tag is looked at: left alone the compiler moves the word's read behind the check -- it is read
        //  again after a tile fetch anyway -- and a batch pays one more LDS round trip)
        asm volatile("; tile word %0 and tag %1" : "+v"(word_r), "+v"(tagv));
        if (ballot64(inb & (tagv != tile_key(tx, ty)))) {
            if (!ensure_tiles(c, inb, nx, ny)) {         // slot conflict: one entry at a time
                cnt = 1;
                valid = e < cnt;
                inb = inb && valid;
                ensure_tiles(c, inb, nx, ny);
            }
            word_r = G_TW(wave)[cell];
        }
        const bool cand = inb & ((word_r & 3u) == 0u);   // :537: not in curMap, not banned (2 is growable, Q5)
        const unsigned long long candm = ballot64(cand);
        DSTAT(ST_BATCHES, 1);
        [[maybe_unused]] const long long bt1 = NOW();
        BSTAT(ST_TRECT, bt1 - bt0);
        [[maybe_unused]] long long bt2 = bt1, bt3 = bt1;
        if (candm) {
            const int q = ny * w + nx;
            const float af = __uint_as_float(word_r & ~3u);
            float sf, cf;
            fast_sincos(af, sf, cf);
            // first occurrence of every candidate pixel: a lane is a repeat iff an EARLIER entry of the batch
            // has the pixel in its 3x3 neighbourhood (that entry's lane for it comes first in reference order)
            bool winner = cand;
            if (cnt > 1) {
                const int ex0 = (int)(pk & 0xffffu), ey0 = (int)(pk >> 16);
                for (int e2 = 0; e2 + 1 < cnt; e2++) {
                    const int px2 = __builtin_amdgcn_readlane(ex0, e2 * 8), py2 = __builtin_amdgcn_readlane(ey0, e2 * 8);
                    winner = winner & !((e > e2) & ((unsigned)(nx - px2 + 1) <= 2u) & ((unsigned)(ny - py2 + 1) <= 2u));
                }
            }
            unsigned long long gone = 0;                 // every lane whose pixel became a member in this batch
            bool bulk = false;
            float dot = 0.0f;
            bt2 = NOW();
            BSTAT(ST_TNFA, bt2 - bt1);
            if (tol_small) {
                const float m = (float)__builtin_popcountll(ballot64(winner));
                dot = __builtin_fmaf(cf, Cf, sf * Sf);                            // ~ cos(distance) * |V|
                const float eps_c = kEpsU * (1.0f + 2.1f * nrat) + 5e-6f;         // incl. the error of Vn
                // a candidate is compared with the sum after the winners BEFORE it (at most m - 1) have been added, each turning it by
                // at most turn / |V| (|V| >= 1 here: accepted vectors only lengthen the sum); a lone candidate sees no drift at all
                const float delta = (m - 1.0f) * turn * rV + 1e-7f;
                const float t_hi = delta <= tolf_lo ? (cos_tol + delta * sin_tol + eps_c) * Vn : 3e38f;
                const float t_lo = delta <= 1.6f ? (cos_tol - delta * fminf(1.0f, sin_tol + delta) - eps_c) * Vn : -3e38f;
                const unsigned long long pcm = ballot64(cand & (dot > t_hi));     // candidates that clearly pass
                const unsigned long long failm = ballot64(cand & (dot < t_lo));   // ... clearly fail
                bulk = (candm & ~(pcm | failm)) == 0ull;
                if (bulk && pcm) {
                    const unsigned long long P = ballot64(winner) & pcm;
                    const int np = __builtin_popcountll(P);
                    if ((P >> lane) & 1ull) {
                        const int idx = n + mbcnt(P);
                        G_TW(wave)[cell] = word_r | 2u;                           // :549
                        G_LST(wave)[idx & LMASK] = pack_xy(nx, ny);               // :551-556
                        if (wt) spill[(uint32_t)idx] = pack_xy(nx, ny);
                    }
                    float ps = 0.0f, pc2 = 0.0f;
                    unsigned long long todo = P;
                    while (todo) {
                        const int l = __builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        pc2 += rlf(cf, l); ps += rlf(sf, l);
                    }
                    Ce += (double)pc2; Se += (double)ps;
                    n += np;
                    flt_valid = false;                   // the region angle moved
                    gone = pcm;
                }
            }
            if (!bulk) {
                // ---- pixel by pixel, in reference order (lane order) ----
                unsigned long long todo = candm;
                while (todo) {
                    int l, decided = -1;                 // 1 take, 0 reject, -1 exact test needed
                    if (tol_small) {
                        // All candidates still to come, against the estimate as it stands: the ones that clearly fail BEFORE the
                        // first one that does not are decided for good (nothing is accepted in between, so this is the estimate
                        // they meet at their turn) -- the loop runs once per accepted pixel, not once per candidate.
                        const float Cg = (float)Ce, Sg = (float)Se;
                        const float Vg = __builtin_amdgcn_sqrtf(Cg * Cg + Sg * Sg) * 1.000001f;
                        const float nr = (float)n * inv_ub(fmaxf(Vg, 1e-3f));
                        const float ec = kEpsU * (1.0f + 2.1f * nr) + 5e-6f;
                        const float d1 = cf * Cg + sf * Sg;
                        const unsigned long long failm1 = ballot64(d1 < (cos_tol - ec) * Vg);
                        const unsigned long long passm1 = ballot64(d1 > (cos_tol + ec) * Vg);
                        const unsigned long long nf = todo & ~(failm1 | gone);
                        if (!nf) break;                  // everything left fails
                        l = __builtin_ctzll(nf);
                        todo &= ~((2ull << l) - 1ull);   // (l < 63 or the mask is all ones: 2 << 63 wraps to 0)
                        if ((passm1 >> l) & 1ull) decided = 1;
                    } else {
                        l = __builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        if ((gone >> l) & 1ull) continue;    // the same pixel was accepted a moment ago
                        const float Cg = (float)Ce, Sg = (float)Se;
                        const float Vg = __builtin_amdgcn_sqrtf(Cg * Cg + Sg * Sg) * 1.000001f;
                        const float nr = (float)n * inv_ub(fmaxf(Vg, 1e-3f));
                        if (Vg > 0.05f) {
                            // any tolerance: the reference's wrapped difference (:540-542) of estimates, exact when near a discontinuity
                            const double R = n == 1 ? regDeg0 : atan2(Se, Ce);
                            const double er = (n == 1 ? 0.0 : (double)(1.05f * kEpsU * nr) + 1e-7) + 1.2e-6;   // + the packed angle's own error
                            const double al = (double)rlf(af, l);
                            const double rw = fabs(R - al);
                            const double df = rw > kPi * 3 / 2.0 ? fabs(rw - 2.0 * kPi) : rw;
                            if (!(fabs(R) > kPi - er || fabs(df - tol) <= er || fabs(rw - kPi * 3 / 2.0) <= er)) decided = df < tol ? 1 : 0;
                        }
                        decided = uni(decided);          // (the same in every lane; computed on the vector unit)
                    }
                    const float cl = rlf(cf, l), sl = rlf(sf, l);
                    const int ql = __builtin_amdgcn_readlane(q, l);
                    if (decided < 0) {
                        g_ctx[wave].llo = wt ? max(n - LCAP, 0) : 0;              // (all lanes, same value: what exact_sums()'s reads go by)
                        exact_sums(c.wave, n);
                        const double R = n == 1 ? regDeg0 : atan2_g(g_ws[wave].ex_sin, g_ws[wave].ex_cos);   // :547 (regDeg is the seed's angle until the first accept)
                        DSTAT(ST_EXACT, 1);
                        const double dq = c.deg[ql], adq = angle_diff(R, dq);
                        decided = uni(adq < tol ? 1 : 0);                                   // :540-543
                        {   // within the libm's noise of the tolerance, or of the wrap at 3 pi / 2?  (tol == 0 and equal angles: an exact 0 < 0 on any libm)
                            const double es = g_ws[wave].ex_sin, ec = g_ws[wave].ex_cos;
                            const double nz = kTieAng * (1.0 + (n == 1 ? 0.0 : (double)n / fmax(sqrt(es * es + ec * ec), 1e-300)));
                            // (the wrap at 3 pi / 2 (:541) maps a difference that fails to one of pi / 2, which fails as well unless tol reaches a quarter turn)
                            // (angles that are 0, +-pi/2 or +-pi to the last bit -- axis-parallel walls -- are the same constants on every libm)
                            const bool quarters = (R == 0.0 || fabs(R) == kPi / 2.0 || fabs(R) == kPi) && (dq == 0.0 || fabs(dq) == kPi / 2.0 || fabs(dq) == kPi);
                            const bool tie = !quarters && ((fabs(adq - tol) <= nz && !(tol == 0.0 && adq == 0.0)) || (tol > 1.5 && fabs(fabs(R - dq) - kPi * 3 / 2.0) <= nz));
                            TIES_AT(TS_GROW, uni(tie ? 1 : 0));
                        }
                    }
                    if (decided == 1) {
                        if (lane == l) {
                            G_TW(wave)[cell] = word_r | 2u;                       // :549
                            G_LST(wave)[n & LMASK] = pack_xy(nx, ny);             // :551-556
                            if (wt) spill[(uint32_t)n] = pack_xy(nx, ny);
                        }
                        Ce += (double)cl; Se += (double)sl;
                        n++;
                        flt_valid = false;
                        gone |= ballot64(cand & (q == ql));
                    }
                }
            }
            bt3 = NOW();
            BSTAT(ST_TMARK, bt3 - bt2);
            // entries that still have a growable non-member neighbour go to the next sweep's worklist
            const unsigned long long left = candm & ~gone;
            if (filter && left) {
                const bool has = valid & (((left >> (8 * e)) & 0xffull) != 0ull);
                if (tol_small) {
                    // slack of this entry's remaining candidates: sin(distance - tol), from the start-of-batch estimate;
                    // after a pixel-by-pixel batch the sum has moved in between, so no slack is claimed (0 = test in full next time)
                    float sg = 2.0f;
                    if ((left >> lane) & 1ull) {
                        if (bulk) {
                            const float ct = fminf(fmaxf(dot * rV, -1.0f), 1.0f);
                            const float st = __builtin_amdgcn_sqrtf(fmaxf(0.0f, 1.0f - ct * ct));
                            const float cs_ = ct * cos_tol + st * sin_tol;            // cos(distance - tol)
                            sg = cs_ <= 0.0f ? 1.0f : st * cos_tol - ct * sin_tol;    // sin(distance - tol), 1 beyond a quarter turn
                        } else sg = 0.0f;
                    }
                    sg = min8(sg);
                    if (has && k == 0 && eidx < mcap)
                        meta[(uint32_t)eidx] = nf4{Cf * rV, Sf * rV, sg - 1.2e-4f - 8.0f * kEpsU * nrat, 0.0f};
                }
                const unsigned long long hm = ballot64(has & (k == 0));
                const int add = __builtin_popcountll(hm);
                const bool room = nxt_cnt + add <= WCAP && n <= 65535;
                // (in place: the next worklist never passes the read cursor -- every entry written was read before, in this batch or earlier)
                G_WL(wave)[(room & has & (k == 0)) ? nxt_cnt + mbcnt(hm) : WCAP] = (uint16_t)eidx;   // (no branch: dummy slot)
                filter = filter && room;
                nxt_cnt += room ? add : 0;
            }
            BSTAT(ST_TREFINE, NOW() - bt3);
        }
        bt_last = NOW();
        return cnt;
    };
    // The loop state is wave-uniform by construction, but the compiler's divergence analysis gives up on it as soon as the
    // join of some lane-conditional store coincides with a join of the uniform control flow (which its CFG simplifications
    // produce at will) -- and then runs the whole loop as divergent code on the vector unit.  Saying it again at the top of
    // every iteration costs nothing where the analysis already knows, and keeps the control flow scalar where it does not.
#define GROW_ESTIMATE()                                                                                                   \
    n = uni(n); nxt_cnt = uni(nxt_cnt); filter = uni((int)filter) != 0; wt = uni((int)wt) != 0;                          \
    if (!wt && n + 64 > LCAP) {             /* the batch to come may wrap the ring: from here on the list is in HBM as well */ \
        for (int k2 = lane; k2 < n; k2 += 64) spill[(uint32_t)k2] = G_LST(wave)[k2];                                      \
        wg_fence();                                                                                                       \
        wt = true;                                                                                                        \
    }                                                                                                                     \
    const float Cf = (float)Ce, Sf = (float)Se;                      /* the estimate of this batch (same in every lane) */ \
    const float V2 = __builtin_fmaf(Cf, Cf, Sf * Sf);                                                                     \
    const float rV = __builtin_amdgcn_rsqf(fmaxf(V2, 1e-12f)) * 1.000001f;   /* >= 1 / |V| */                             \
    const float Vn = V2 * rV;                                                 /* |V| (to 2e-6) */                          \
    const float nrat = (float)n * rV;                                         /* >= n / |V| */
    int sweep = 1, ex;
    do {                                                     // :525 sweeps to fixpoint (Q7)
        ex = n;
        nxt_cnt = 0;
        int i = n;                                           // contiguous cursor: the entries appended during this sweep ...
        // ... or the whole list: the first sweep; worklists given up; and a region of up to 8 pixels -- one batch sweeps it
        // again, which costs less than fetching the slack records of its worklist (most regions are this small)
        if (sweep == 1 || !filter || n <= 8) i = 0;
        else {
            // ---- entries of earlier sweeps that still had a growable non-member neighbour ----
            int wi = 0;                                      // worklist cursor
            while (true) {
                GROW_ESTIMATE();
                wi = uni(wi); wl_cnt = uni(wl_cnt); flt_base = uni(flt_base); flt_valid = uni((int)flt_valid) != 0;
                flt_need = ((unsigned long long)(uint32_t)uni((int)(uint32_t)(flt_need >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)flt_need);
                if (wi >= wl_cnt) break;
                int cnt = min(8, wl_cnt - wi);
                if (tol_small && filter) {                   // (filter lost in this sweep: the rest of the worklist is tested in full)
                    if (!flt_valid || wi >= flt_base + 64) {
                        flt_base = wi;
                        bool nd = false;
                        if (wi + lane < wl_cnt) {
                            const int ei = (int)G_WL(wave)[wi + lane];
                            nd = true;
                            if (ei < mcap) {
                                const nf4 mt = meta[(uint32_t)ei];
                                const float vx = Cf * rV, vy = Sf * rV;                  // current unit sum vector (norm within 3e-6 of 1)
                                const float dotv = mt.x * vx + mt.y * vy, crs = fabsf(mt.x * vy - mt.y * vx);
                                nd = !(dotv > 0.0f && crs + 1e-5f + 2.0f * kEpsU * nrat < mt.z);
                            }
                        }
                        flt_need = ballot64(nd);
                        flt_valid = true;
                    }
                    const int off = wi - flt_base;
                    const int nval = min(64, wl_cnt - flt_base) - off;         // entries of the chunk from wi on
                    const unsigned long long rest = flt_need >> off;          // bit 0 = entry wi
                    const int nskip = rest ? min(__builtin_ctzll(rest), nval) : nval;
                    if (nskip > 0) {                         // a run of entries that cannot accept anything: carry them over
                        // (lane-dependent branches stay in the MIDDLE of wave-uniform blocks, see STAT)
                        const bool room = nxt_cnt + nskip <= WCAP;
                        // (in place: all 64 lanes read before any of them writes, and nxt_cnt <= wi)
                        G_WL(wave)[room && lane < nskip ? nxt_cnt + lane : WCAP] = G_WL(wave)[min(wi + lane, WCAP - 1)];   // (no branch: dummy slot)
                        filter = filter && room;
                        nxt_cnt += room ? nskip : 0;
                        wi += nskip;
                        continue;
                    }
                    // the run of consecutive entries to test (no skipped entry in between: its check would be stale after an accept)
                    const unsigned long long inv = ~rest;
                    cnt = min(cnt, inv ? __builtin_ctzll(inv) : 64);
                }
                // (the address is built from a scalar the compiler cannot see through: left alone it keeps "worklist + 2 e" in a register across
                //  the whole sweep, which at 128 registers is a scratch reload in front of every batch)
                uint32_t wl_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)(G_WL(wave) + wi);
                asm volatile("; worklist cursor %0" : "+s"(wl_at));
                const int eidx = e < cnt ? (int)*(__attribute__((address_space(3))) const uint16_t*)(uintptr_t)(wl_at + 2u * (uint32_t)e) : 0;
                wi += batch(cnt, eidx, false, Cf, Sf, rV, Vn, nrat);
            }
        }
        while (true) {                                       // ---- contiguous entries; n is live (:529) ----
            GROW_ESTIMATE();
            i = uni(i);
            if (i >= n) break;
            const int cnt = min(8, n - i);
            i += batch(cnt, i + e, n - i <= LCAP, Cf, Sf, rV, Vn, nrat);   // (direct: entries i .. n - 1 are all in the ring)
        }
        wl_cnt = nxt_cnt;
        sweep++;
        flt_valid = false;
        if (n != ex && n > 8) wg_fence();                    // meta[] written in this sweep is read in the next
    } while (n != ex);
#undef GROW_ESTIMATE
    if (lane == 0) { g_ws[wave].gnum = n; g_ctx[wave].llo = wt ? max(n - LCAP, 0) : 0; }
    if (wt) wg_fence();                                      // the written-through part is read back by the stages that follow
    STAT(ST_GROW, 1);
    STAT(ST_GROWN, n);
    if (!tol_small) STAT(ST_GROWANY, 1);
    DSTAT(ST_TGROW, NOW() - t0);
    return n;
}
// The two out-of-line functions eval_seed() chooses between by the wave-uniform tolerance (region/eval.h)
__device__ __noinline__ int grow(int cw_, int sx_, int sy_, double regDeg0_, double tol_) { return grow_body<true>(cw_, sx_, sy_, regDeg0_, tol_); }        // tol < 1.5
__device__ __noinline__ int grow_any(int cw_, int sx_, int sy_, double regDeg0_, double tol_) { return grow_body<false>(cw_, sx_, sy_, regDeg0_, tol_); }   // every other tolerance (counted: ST_GROWANY)
