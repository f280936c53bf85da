// region/rect.h -- the rectangle of a grown region: rect_convert = CenterGetter (myLSD.cpp:592-619) + OrientationGetter (:621-667) + RectangleConverter
// (:669-734), rec_density, and radius_reduce = RegionRadiusReducer (:736-802).  Reads the list (lget) and g_acc, writes g_ws[].rec; the Reducer empties the
// tile cache into tmask (flush_tiles), reorders the list and uses the arena behind the list ring (kMvCap words) as scratch.
__device__ __noinline__ void rect_convert(int cw_, int num, double regdeg, double aliPro, int pk, double tol) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int lane = c.lane, w = c.w;
    [[maybe_unused]] const long long t0 = NOW();
    const int wave = __builtin_amdgcn_readfirstlane(c.wave);
    double S = 0;                                // serial accumulation in list order (bit-exact): lane 0 cenX, 1 cenY, 2 weight sum
    for (int base = 0; base < num; base += 64) {                                   // :608-613
        const int kx = base + lane;
        const bool valid = kx < num;
        const uint32_t pkx = valid ? lget(c, kx) : 0u;
        const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
        const double wgt = valid ? c.mag[(size_t)y * w + x] : 0.0;
        const double ax = wgt * x, ay = wgt * y;
        for (int half = 0; half < kStageRounds; half++) {
            const int cnt = min(kStage, num - base - kStage * half);
            if (cnt <= 0) break;
            stage4(wave, lane, half, ax, ay, wgt, 0.0);
            S = acc32(wave, lane, cnt, S);
        }
    }
    double ws = rl(S, 2);
    const double cenX = rl(S, 0) / ws;
    const double cenY = rl(S, 1) / ws;

    S = 0;                                       // lane 0 Ixx, 1 Iyy, 2 Ixy, 3 weight sum
    for (int base = 0; base < num; base += 64) {                                   // :637-643
        const int kx = base + lane;
        const bool valid = kx < num;
        const uint32_t pkx = valid ? lget(c, kx) : 0u;
        const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
        const double wgt = valid ? c.mag[(size_t)y * w + x] : 0.0;
        const double ddy = y - cenY, ddx = x - cenX;
        const double a = wgt * (ddy * ddy), b = wgt * (ddx * ddx), cc = wgt * ddx * ddy;
        for (int half = 0; half < kStageRounds; half++) {
            const int cnt = min(kStage, num - base - kStage * half);
            if (cnt <= 0) break;
            stage4(wave, lane, half, a, b, -cc, wgt);     // Ixy -= cc (:642): adding the negated term is the same operation
            S = acc32(wave, lane, cnt, S);
        }
    }
    ws = rl(S, 3);
    const double Ixx = rl(S, 0) / ws, Iyy = rl(S, 1) / ws, Ixy = rl(S, 2) / ws;
    const double dI = Ixx - Iyy;
    const double lamb = (Ixx + Iyy - sqrt(dI * dI + 4 * Ixy * Ixy)) / 2.0;          // :647
    double inertiaDeg;
    {
        const bool xx = fabs(Ixx) > fabs(Iyy);                                    // :649-652
        inertiaDeg = atan2_g(xx ? lamb - Ixx : Ixy, xx ? Ixy : lamb - Iyy);
    }
    double regDif = inertiaDeg - regdeg;                                          // :655-665
    while (regDif <= -kPi) regDif += 2 * kPi;
    while (regDif > kPi) regDif -= 2 * kPi;
    if (regDif < 0) regDif = -regDif;
    TIES_AT(TS_FLIP, fabs(regDif - tol) <= kTieFlip ? 1 : 0);     // (the wraps above are continuous in |regDif|: no decision)
    if (regDif > tol) inertiaDeg += kPi;

    double dx, dy;
    sincos_g(inertiaDeg, dy, dx);                                                  // :699-700
    double lenMin = 0, lenMax = 0, widMin = 0, widMax = 0;                         // Q9: start at 0 (:701)
    for (int base = 0; base < num; base += 64) {
        const int kx = base + lane;
        if (kx < num) {
            const uint32_t pkx = lget(c, kx);
            const int x = (int)(pkx & 0xffffu), y = (int)(pkx >> 16);
            const double len = (x - cenX) * dx + (y - cenY) * dy;                  // :704
            const double wid = -(x - cenX) * dy + (y - cenY) * dx;                 // :705
            lenMin = fmin(lenMin, len); lenMax = fmax(lenMax, len);
            widMin = fmin(widMin, wid); widMax = fmax(widMax, wid);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {   // min/max are order-independent: plain wave reduction
        lenMin = fmin(lenMin, __shfl_xor(lenMin, off));
        lenMax = fmax(lenMax, __shfl_xor(lenMax, off));
        widMin = fmin(widMin, __shfl_xor(widMin, off));
        widMax = fmax(widMax, __shfl_xor(widMax, off));
    }
    if (lane == 0) {
        Rec& r = g_ws[c.wave].rec;
        r.x1 = cenX + lenMin * dx; r.y1 = cenY + lenMin * dy;                      // :717-720
        r.x2 = cenX + lenMax * dx; r.y2 = cenY + lenMax * dy;
        r.wid = widMax - widMin;
        r.cX = cenX; r.cY = cenY; r.deg = inertiaDeg; r.dx = dx; r.dy = dy;
        r.p = aliPro; r.prec = tol; r.pk = pk;
        if (r.wid < 1) r.wid = 1;                                                  // :730
    }
    PSTAT(ST_TRECT, NOW() - t0);
}

__device__ __forceinline__ double rec_density(int num, const Rec& r) {             // :757,:798,:827,:867
    const double ex = r.x1 - r.x2, ey = r.y1 - r.y2;
    return num / (sqrt(ex * ex + ey * ey) * r.wid);
}

// ---------------------------------------------------------------------------------------------
// RegionRadiusReducer, myLSD.cpp:736-802 (incl. the `i <= num` sentinel behaviour)
// ---------------------------------------------------------------------------------------------
// Returns the new region size, or -(size + 1) when the region is given up (:792).  The rectangle is g_ws[c.wave].rec.
__device__ __noinline__ int radius_reduce_impl(int cw_, int sx, int sy, int num, double regdeg, double denThre);
__device__ __noinline__ int radius_reduce(int cw_, int sx, int sy, int num, double regdeg, double denThre) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    [[maybe_unused]] const long long t0 = NOW();
    const int r = radius_reduce_impl(c.wave, sx, sy, num, regdeg, denThre);
    return r;
}
__device__ __noinline__ int radius_reduce_impl(int cw_, int sx, int sy, int num, double regdeg, double denThre) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int lane = c.lane;
    STAT(ST_RRR, 1);
    double den = rec_density(num, g_ws[c.wave].rec);
    const bool axis0 = axis_exact(g_ws[c.wave].rec.dx, g_ws[c.wave].rec.dy);
    // (the comparison with denThre here repeats the caller's, which has counted its tie; the ones after a refit are counted below)
    if (den > denThre) return num;                                                 // :760
    // keep the grow-order list for the marking loops before it gets reordered
    for (int k2 = lane; k2 < num; k2 += 64) c.gcopy[k2] = lget(c, k2);
    // curMap moves to HBM in full: the removals below clear bits there, the marking stages read them there (and the scratch of the
    // parallel passes takes the tile cache's place)
    flush_tiles(c);
    if (lane == 0) g_ws[c.wave].has_copy = 1;
    wg_fence();
    const Rec rec = g_ws[c.wave].rec;
    const double ax = sx - rec.x1, ay = sy - rec.y1, bx = sx - rec.x2, by = sy - rec.y2;
    const double rad1 = sqrt(ax * ax + ay * ay), rad2 = sqrt(bx * bx + by * by);    // :768-769
    double rad = rad1 > rad2 ? rad1 : rad2;
    bool removed_any = false;
    const int wave = __builtin_amdgcn_readfirstlane(c.wave);
    unsigned long long* const msk = reinterpret_cast<unsigned long long*>(g_acc[wave]);   // keep-masks of up to kStage * 4 chunks of 64 entries
    uint32_t* const mv = reinterpret_cast<uint32_t*>(G_WL(wave));                          // up to kMvCap moved entries: the worklist and the tile cache behind it
    while (den < denThre) {                                                        // :775
        rad *= 0.75;
        STAT(ST_RRRPASS, 1);
        num = __builtin_amdgcn_readfirstlane(num);
        // The reference walks the list from the front and fills every slot whose point is farther than rad with the LAST
        // point of the list, re-testing it (:779-789).  The outcome is: the K points within rad stay in slots [0, K); the
        // holes among those slots (ascending) receive the kept points of the slots >= K, taken from the back (descending).
        // That is computed 64 entries at a time; lists too long for the scratch arrays take the reference's own loop below.
        const int nchunks = (num + 63) >> 6;
        bool parallel = nchunks <= kStage * 4;
        int K = 0;
        if (parallel) {
            for (int ci = 0; ci < nchunks; ci++) {
                const int idx = ci * 64 + lane;
                const bool valid = idx < num;
                const uint32_t pkx = valid ? lget(c, idx) : 0u;
                const int px = (int)(pkx & 0xffffu), py = (int)(pkx >> 16);
                const double ddx = sx - px, ddy = sy - py;
                const double dist = sqrt(ddx * ddx + ddy * ddy);
                const bool far = valid & (dist > rad);                             // :780
                if (!axis0) TIES_AT(TS_DIST, __builtin_popcountll(ballot64(valid & (fabs(dist - rad) <= kTieRel * (1.0 + rad)))));   // (rad derives from the rectangle's corners)
                const unsigned long long nearm = ballot64(valid & !far);
                msk[ci] = nearm;                           // (all lanes, same value)
                K += __builtin_popcountll(nearm);
            }
            if (min(K, num - K) > kMvCap) parallel = false;  // more moves than mv[] holds
        }
        if (parallel) {
            if (K != num) {
                int nm = 0;                                // kept points of the slots >= K, highest slot first
                for (int ci = nchunks - 1; ci >= 0 && ci * 64 + 63 >= K; ci--) {
                    const int idx = ci * 64 + lane;
                    const bool is = (((msk[ci] >> lane) & 1ull) != 0ull) & (idx >= K);
                    const unsigned long long mm = ballot64(is);
                    const int above = __builtin_popcountll((mm >> lane) >> 1);
                    mv[is ? nm + above : kMvCap] = is ? lget(c, idx) : 0u;         // (no branch: dummy slot)
                    nm += __builtin_popcountll(mm);
                }
                int nh = 0;                                // far points of the slots < K, lowest slot first
                for (int ci = 0; ci * 64 < K; ci++) {
                    const int idx = ci * 64 + lane;
                    const bool valid = idx < num;
                    const bool nearb = ((msk[ci] >> lane) & 1ull) != 0ull;
                    const unsigned long long hm = ballot64((idx < K) & !nearb);
                    const uint32_t old = valid ? lget(c, idx) : 0u;
                    if (valid & !nearb) tm_clear(c, (int)(old & 0xffffu), (int)(old >> 16));       // curMap = 0 (:781), every far point of this chunk
                    if ((idx < K) & !nearb) lset(c, idx, mv[nh + mbcnt(hm)]);                      // :782-785
                    nh += __builtin_popcountll(hm);
                }
                for (int ci = (K + 63) >> 6; ci < nchunks; ci++) {                                 // far points of the chunks wholly behind K
                    const int idx = ci * 64 + lane;
                    if ((idx < num) & (((msk[ci] >> lane) & 1ull) == 0ull)) {
                        const uint32_t old = lget(c, idx);
                        tm_clear(c, (int)(old & 0xffffu), (int)(old >> 16));
                    }
                }
                num = K;
                removed_any = true;
            }
            // the extra round at i == num (:779 `<=`): the slot holds the NULL written at :784-785, i.e. the point (0, 0)
            if (!removed_any) STAT(ST_OOB, 1);             // the reference reads out of bounds here (UB): no removal
            else {
                const double ddx = sx, ddy = sy;
                if (!axis0) TIES_AT(TS_DIST, fabs(sqrt(ddx * ddx + ddy * ddy) - rad) <= kTieRel * (1.0 + rad) ? 1 : 0);
                if (sqrt(ddx * ddx + ddy * ddy) > rad) {
                    if (lane == 0) tm_clear(c, 0, 0);      // curMap(0, 0) = 0
                    num--;                                 // the last point is dropped from the list (its curMap bit stays)
                    STAT(ST_SENT, 1);
                }
            }
            wg_fence();
        }
        int i = parallel ? num + 1 : 0;
        while (i <= num) {                                                         // :779 (`<=`)
            int px, py;
            if (i == num) {
                if (!removed_any) { STAT(ST_OOB, 1); break; }   // the reference reads out of bounds here (UB): no removal
                px = 0; py = 0;                            // slot holds the NULL written at :784-785
            } else {
                const uint32_t pkx = lget(c, i);
                px = (int)(pkx & 0xffffu); py = (int)(pkx >> 16);
            }
            const double ddx = sx - px, ddy = sy - py;
            if (!axis0) TIES_AT(TS_DIST, fabs(sqrt(ddx * ddx + ddy * ddy) - rad) <= kTieRel * (1.0 + rad) ? 1 : 0);
            if (sqrt(ddx * ddx + ddy * ddy) > rad) {                               // :780
                if (lane == 0) {
                    tm_clear(c, px, py);                                           // curMap = 0 (:781)
                    if (i == num) { lset(c, num - 1, 0u); }
                    else { lset(c, i, lget(c, num - 1)); lset(c, num - 1, 0u); }   // :782-785
                }
                if (i == num) STAT(ST_SENT, 1);
                wg_fence();
                removed_any = true;
                i--;
                num--;
            }
            i++;
        }
        if (num < 2) return -(num + 1);                                            // :792
        rect_convert(c.wave, num, regdeg, rec.p, rec.pk, rec.prec);                     // :797 (p, prec unchanged)
        den = rec_density(num, g_ws[c.wave].rec);
        TIES_AT(TS_DENS, (fabs(den - denThre) <= kTieRel * denThre && !axis_exact(g_ws[c.wave].rec.dx, g_ws[c.wave].rec.dy)) ? 1 : 0);       // :775
    }
    return num;
}
