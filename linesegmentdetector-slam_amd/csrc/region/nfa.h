// region/nfa.h -- LogGammaCalculator (myLSD.cpp:882-924), RectangleNFACalculator (:926-1059, as nfa_count + nfa_tail) and RectangleImprover (:1061-1158,
// improve).  nfa_count keeps its column scan in the worklist's place of the arena (G_WL); improve works on g_ws[].rec and the counters (g_stat).
// LogGammaCalculator (:882-924): a look-up in the host-computed table (lsd_ctx.hip sizes it for every pixel count a rectangle of
// the image can have; only images of more than kLgTableMax scaled pixels can get past it, and then with the device's own log / sinh / pow)
__device__ __forceinline__ double log_gamma_dev(const double* lgamma, int lg_count, int x) {
    if (x >= 0 && x < lg_count) return lgamma[x];
    const double xd = x;
    return 0.918938533204673 + (xd - 0.5) * log(xd) - xd +
           0.5 * xd * log(xd * sinh(1.0 / xd) + 1.0 / (810 * pow(xd, 6.0)));
}

// ---------------------------------------------------------------------------------------------
// RectangleNFACalculator, myLSD.cpp:926-1059 (the full-image pass :940-945 is a no-op, not restated), in two parts: the pixel
// count of the rectangle with all 64 lanes (:947-1017), and the value from the two counts (:1019-1058) -- scalar arithmetic that
// RectangleImprover's five tries of a phase run side by side in five lanes (improve(), below).
// ---------------------------------------------------------------------------------------------
// Returns `all`; ali[q] = pixels of the rectangle whose level-line angle is within prec[q] of the rectangle's (NP > 1: the tries of
// a phase that halves p share the rectangle and differ in the precision only).
template <int NP>
__device__ __forceinline__ int nfa_count(const RCtx& c, const Rec& rec, const double (&prec)[NP], int (&ali)[NP]) {
    const int lane = c.lane, xLim = c.w, yLim = c.h;
    STAT(ST_NFA, NP);
    [[maybe_unused]] const long long t00 = NOW();
    double verX[4], verY[4];
    verX[0] = rec.x1 - rec.dy * rec.wid / 2.0;                                     // :949-956
    verX[1] = rec.x2 - rec.dy * rec.wid / 2.0;
    verX[2] = rec.x2 + rec.dy * rec.wid / 2.0;
    verX[3] = rec.x1 + rec.dy * rec.wid / 2.0;
    verY[0] = rec.y1 + rec.dx * rec.wid / 2.0;
    verY[1] = rec.y2 + rec.dx * rec.wid / 2.0;
    verY[2] = rec.y2 - rec.dx * rec.wid / 2.0;
    verY[3] = rec.y1 - rec.dx * rec.wid / 2.0;
    int offset;
    if ((rec.x1 < rec.x2) && (rec.y1 <= rec.y2)) offset = 0;                       // :959-966
    else if ((rec.x1 >= rec.x2) && (rec.y1 < rec.y2)) offset = 1;
    else if ((rec.x1 > rec.x2) && (rec.y1 >= rec.y2)) offset = 2;
    else offset = 3;
    const double vx0 = verX[offset & 3], vx1 = verX[(offset + 1) & 3], vx2 = verX[(offset + 2) & 3],
                 vx3 = verX[(offset + 3) & 3];
    const double vy0 = verY[offset & 3], vy1 = verY[(offset + 1) & 3], vy2 = verY[(offset + 2) & 3],
                 vy3 = verY[(offset + 3) & 3];
    const double cx0 = ceil(vx0);
    int xlen = cvt_x86(cx0 - floor(vx2));                                          // :973
    if (xlen < 0 && xlen != (int)0x80000000) xlen = -xlen;
    xlen = (int)((unsigned)xlen + 1u);
    const double k0 = (vy1 - vy0) / (vx1 - vx0);                                   // :979-982
    const double k1 = (vy2 - vy1) / (vx2 - vx1);
    const double k2 = (vy2 - vy3) / (vx2 - vx3);
    const double k3 = (vy3 - vy0) / (vx3 - vx0);
    int all = 0;
    #pragma unroll
    for (int q = 0; q < NP; q++) ali[q] = 0;
    // decisions within the libm's noise (ST_TIES): a corner or an edge within kTieCoord of a pixel column / row (not for rectangles that
    // are axis-parallel to the last bit: their coordinates do not depend on the libm), a pixel's angle within kTieAng-ish of the precision
    const bool axis0 = axis_exact(rec.dx, rec.dy);
    const double ex_ = rec.x2 - rec.x1, ey_ = rec.y2 - rec.y1;
    const double cnz = kTieCoord * (fabs(rec.x1) + fabs(rec.y1) + fabs(ex_) + fabs(ey_) + rec.wid + 1.0);     // what the libm's last place can move a corner
    int ties_a = 0;
    int ties = (lane == 0 && !axis0 && (fabs(vx0 - rint(vx0)) <= cnz || fabs(vx2 - rint(vx2)) <= cnz)) ? 1 : 0;   // (per lane; summed over the wave below)
    // per-column scan results of one 64-column block; the sweep worklists are free while a rectangle is being rated
    int* const s_incl = reinterpret_cast<int*>(G_WL(c.wave));
    int* const s_lo = s_incl + 64;
    int* const s_x = s_incl + 128;
    for (int cb = 0; cb < xlen; cb += 64) {
        const int i = cb + lane;
        int cntc = 0, lo = 0, xr = 0;
        if (i < xlen) {
            xr = cvt_x86(i + cx0);                                                 // :976
            int yLow, yHigh;
            const double eLow = xr < vx3 ? vy0 + (xr - vx0) * k3 : vy3 + (xr - vx3) * k2;     // :988-989 / :992-993
            const double eHigh = xr < vx1 ? vy0 + (xr - vx0) * k0 : vy1 + (xr - vx1) * k1;    // :998-999 / :1002-1003
            yLow = cvt_x86(ceil(eLow));
            yHigh = cvt_x86(floor(eHigh));
            const double kLow = xr < vx3 ? k3 : k2, kHigh = xr < vx1 ? k0 : k1;
            if (!axis0 && (fabs(eLow - rint(eLow)) <= cnz * (1.0 + fabs(kLow)) || fabs(eHigh - rint(eHigh)) <= cnz * (1.0 + fabs(kHigh)) ||
                           fabs(xr - vx3) <= cnz || fabs(xr - vx1) <= cnz)) {
                ties++;
#ifdef LSD_TIE_PRINT
                printf("edge tie: xr %d eLow %.17g eHigh %.17g vx0 %.17g vx1 %.17g vx3 %.17g dx %.17g dy %.17g wid %.17g x1 %.17g y1 %.17g\n", xr, eLow, eHigh, vx0, vx1, vx3, rec.dx, rec.dy, rec.wid, rec.x1, rec.y1);
#endif
            }
            if (xr >= 0 && xr < xLim) {                                            // :1007
                lo = yLow < 0 ? 0 : yLow;
                const int hi = yHigh > yLim - 1 ? yLim - 1 : yHigh;
                if (hi >= lo) cntc = hi - lo + 1;
            }
        }
        int inc = cntc;                                       // inclusive wave scan of the column heights
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (lane >= off) inc += t;
        }
        const int tot = __builtin_amdgcn_readlane(inc, 63);
        if (tot == 0) continue;
        s_incl[lane] = inc; s_lo[lane] = lo; s_x[lane] = xr;
        all += tot;
        for (int t0 = 0; t0 < tot; t0 += 64) {                // flattened (column, row) pairs, 64 per step
            const int t = t0 + lane;
            double df = 1e300;                                 // (no pixel: within no precision)
            if (t < tot) {
                int ci = 0;                                    // smallest ci with s_incl[ci] > t
                for (int step = 32; step >= 1; step >>= 1)
                    if (s_incl[ci + step - 1] <= t) ci += step;
                const int ex = ci ? s_incl[ci - 1] : 0;
                const int j = s_lo[ci] + (t - ex);
                df = angle_diff(rec.deg, c.deg[(size_t)j * xLim + s_x[ci]]);       // :1009-1011
            }
            bool near = false;
            #pragma unroll
            for (int q = 0; q < NP; q++) {
                ali[q] += __builtin_popcountll(ballot64(df < prec[q]));            // :1012-1013
                near = near || fabs(df - prec[q]) <= 4.0 * kTieAng;                // (two angles of an ulp each)
            }
            if (near) ties_a++;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) { ties += __shfl_xor(ties, off); ties_a += __shfl_xor(ties_a, off); }
    TIES_AT(TS_EDGE, ties);
    TIES_AT(TS_ALIGN, ties_a);
    PSTAT(ST_NFACNT, NOW() - t00);
    return all;
}

// bit 0 of flags: the value is made of host-computed numbers alone (logNT, log10 p: the reference's own libm) -- no device-evaluated
// function; bits 8..: stopping tests of the tail that the bracket (below) could not decide
struct NfaVal { double v; int flags; };
// Scalar code (every active lane for itself: improve() runs five at a time); p = the rectangle's p, pk the number of its halvings.
__device__ __noinline__ NfaVal nfa_tail(int all, int ali, int pk, double p, double logNT, const double* ptab, const double* lgamma, int lg_count) {
    if (all == 0 || ali == 0) return NfaVal{-logNT, 1};                            // :1019-1022
    const double logp = ptab[pk * 3 + 0], log10p = ptab[pk * 3 + 1], log1mp = ptab[pk * 3 + 2];
    if (all == ali) return NfaVal{-logNT - all * log10p, 1};                       // :1023-1026
    const double proTerm = p / (1.0 - p);
    const double log1Coef = log_gamma_dev(lgamma, lg_count, all + 1) - log_gamma_dev(lgamma, lg_count, ali + 1) - log_gamma_dev(lgamma, lg_count, all - ali + 1);
    const double log1Term = log1Coef + ali * logp + (all - ali) * log1mp;          // :1033
    // From here on the reference calls exp, log10 and pow.  What reaches the result -- the first term and the logarithm of the tail --
    // is evaluated correctly rounded (exp_g, log10_g: crmath.h); pow and log10 inside the loop only decide when the sum stops, and that
    // decision is taken from the device math library's values where a bracket around them (kOcmlBracket, many times their error:
    // tests/test_parity_gpu.py::test_device_libm_is_inside_the_nfa_bracket) leaves no doubt, from the correctly rounded values otherwise.
    double term = exp_g(log1Term);
    const double eps = 2.2204e-16;
    if (fabs(term) < 100 * eps) {                                                  // :1037-1043
        if (ali > all * p) return NfaVal{-log10_g(term) - logNT, 0};
        return NfaVal{-logNT, 1};
    }
    int nslow = 0;
    double binTail = term;
    const double tole = 0.1;
    constexpr double kOcmlBracket = 0x1p-44, kTiny = 0x1p-1000;
    for (int i = ali + 1; i <= all; i++) {                                         // :1046-1056
        const double binTerm = (all - i + 1) / (i * 1.0);
        const double multTerm = binTerm * proTerm;
        term *= multTerm;
        binTail += term;
        if (binTerm < 1) {
            // err < tole * |-log10(binTail) - logNT| * binTail ?  (:1052-1053)  Every operation of the two sides is monotone in the value
            // of pow resp. log10, so the sides at the ends of the brackets enclose the sides at the correctly rounded values.
            const double N = (double)(all - i + 1), om = 1.0 - multTerm;
            const double Pd = pow(multTerm, N), Ld = log10(binTail);
            const double Pe = Pd * kOcmlBracket + kTiny, Le = fabs(Ld) * kOcmlBracket + kTiny;
            const double err_hi = term * ((1 - (Pd - Pe)) / om - 1), err_lo = term * ((1 - (Pd + Pe)) / om - 1);
            const double a1 = -(Ld - Le) - logNT, a2 = -(Ld + Le) - logNT;
            const double f1 = fabs(a1), f2 = fabs(a2);
            const double rhs_hi = tole * fmax(f1, f2) * binTail;
            const double rhs_lo = (a1 > 0) == (a2 > 0) && a1 != 0 && a2 != 0 ? tole * fmin(f1, f2) * binTail : 0.0;
            bool stop;
            if (err_hi < rhs_lo) stop = true;
            else if (!(err_lo < rhs_hi)) stop = false;
            else {
                nslow++;                                    // (stopping tests of the tail the bracket could not decide)
                const double err = term * ((1 - pow_g(multTerm, N)) / om - 1);
                stop = err < tole * fabs(-log10_g(binTail) - logNT) * binTail;
            }
            if (stop) break;
        }
    }
    return NfaVal{-log10_g(binTail) - logNT, nslow << 8};
}

// RectangleImprover, myLSD.cpp:1061-1158: the initial evaluation, then five phases of five tries each.  Within a phase the tried
// rectangles do not depend on the values found (only `best` does, and a phase starts from the best so far): the five pixel
// counts are taken one after the other -- one pass for the phases that only halve p -- and the five values computed side by side.
__device__ __noinline__ double improve(int cw_) {
    RCtx c = g_ctx[__builtin_amdgcn_readfirstlane(cw_)];
    c.lane = (int)(threadIdx.x & 63u);
    const int lane = c.lane;
    const double delt = 0.5, delt2 = delt / 2.0;
    Rec& best = g_ws[c.wave].rec;                           // (the best rectangle so far stays in LDS: every lane writes the same values)
    double bestNFA = 0;
    [[maybe_unused]] const long long t0 = NOW();
    // How close the comparisons below come to a tie, as a MARGIN: the distance of the operands over the most the reference's
    // libm (glibc: exp and pow within 1 ulp, log10 within 1 ulp of the correctly rounded values computed here) can move them apart.
    // v = fl(-L - logNT) with L = log10(tail): |dL| <= 2^-51 |L| + 2^-53 (the tail's first term differs by an ulp), and the
    // subtraction rounds to an ulp of max(|v|, logNT): noise(v) = 2^-51 |v + logNT| + 2^-52 (1 + max(|v|, logNT)).  A decision can come
    // out differently on the two libms only where the margin is below 1 (tools/campaign.py enforces a floor of 2).  A value made of
    // the host's numbers alone (-logNT - n log10 p: an exact 0 exists, w h = 6^4, p = 1/6, n = 10) is the reference's own.
    auto margins = [&](double v, bool host_only, bool first) {
        if (fabs(v) <= 1.7976931348623157e308) {
            const double nv = 0x1p-51 * fabs(v + c.logNT) + 0x1p-52 * (1.0 + fmax(fabs(v), c.logNT));
            if (!host_only) STATMAX(ST_MINNFA, kInfBits - (unsigned long long)__double_as_longlong(fabs(v) / nv));       // (v is compared with 0: :1075, :242)
            int tie = (!host_only && fabs(v) / nv < 2.0) ? 1 : 0;              // (the campaigns' floor: a margin below 1 can flip, below 2 is counted)
            if (!first && v != bestNFA) {
                const double nb = 0x1p-51 * fabs(bestNFA + c.logNT) + 0x1p-52 * (1.0 + fmax(fabs(bestNFA), c.logNT));
                STATMAX(ST_MINGAP, kInfBits - (unsigned long long)__double_as_longlong(fabs(v - bestNFA) / (nv + nb)));
                if (fabs(v - bestNFA) / (nv + nb) < 2.0) tie++;
            }
            TIES_AT(TS_NFA, tie);
        }
    };
    {   // :1075-1079
        Rec r = best;
        const double pr[1] = {r.prec};
        int al[1];
        const int all = nfa_count<1>(c, r, pr, al);
        const NfaVal nv = nfa_tail(all, al[0], r.pk, r.p, c.logNT, c.ptab, c.lgamma, c.lg_count);
        STAT(ST_NFASLOW, nv.flags >> 8);
        margins(nv.v, (nv.flags & 1) != 0, true);
        bestNFA = nv.v;
    }
    // one try of phase ph (:1084-1092 / :1148-1156 halve p; :1097-1107 reduce width; :1112-1125 move one side; :1130-1143 the other)
    auto next_try = [&](Rec& r, int ph) -> bool {
        if (ph == 0 || ph == 4) { r.p /= 2.0; r.prec = r.p * kPi; r.pk++; return true; }
        if (!(r.wid - delt >= 0.5)) return false;
        if (ph == 2) { r.x1 -= r.dy * delt2; r.y1 += r.dx * delt2; r.x2 -= r.dy * delt2; r.y2 += r.dx * delt2; }
        else if (ph == 3) { r.x1 += r.dy * delt2; r.y1 -= r.dx * delt2; r.x2 += r.dy * delt2; r.y2 -= r.dx * delt2; }
        r.wid -= delt;
        return true;
    };
    for (int ph = 0; ph < 5 && !(bestNFA > 0); ph++) {      // phase boundary (:1078,:1093,:1108,:1126,:1144)
        // lane t < 5 keeps the counts of try t
        int my_all = 0, my_ali = 0, my_pk = 0;
        double my_p = 0.0;
        bool my_eval = false;
        Rec r = best;
        if (ph == 0 || ph == 4) {
            double pr[5];
            int al[5];
            #pragma unroll
            for (int t = 0; t < 5; t++) pr[t] = r.p / (double)(2 << t) * kPi;      // p halved t + 1 times, exactly as next_try does it
            const int all = nfa_count<5>(c, r, pr, al);
            #pragma unroll
            for (int t = 0; t < 5; t++)
                if (lane == t) { my_all = all; my_ali = al[t]; my_pk = r.pk + t + 1; my_p = r.p / (double)(2 << t); my_eval = true; }
        } else {
            for (int t = 0; t < 5; t++) {
                if (!next_try(r, ph)) continue;
                const double pr[1] = {r.prec};
                int al[1];
                const int all = nfa_count<1>(c, r, pr, al);
                if (lane == t) { my_all = all; my_ali = al[0]; my_pk = r.pk; my_p = r.p; my_eval = true; }
            }
        }
        NfaVal nv{0.0, 0};
        if (my_eval) nv = nfa_tail(my_all, my_ali, my_pk, my_p, c.logNT, c.ptab, c.lgamma, c.lg_count);
        // the five values in the reference's order
        r = best;
        for (int t = 0; t < 5; t++) {
            if (!next_try(r, ph)) continue;
            const double v = rl(nv.v, t);
            const int fl = __builtin_amdgcn_readlane(nv.flags, t);
            STAT(ST_NFASLOW, fl >> 8);
            margins(v, (fl & 1) != 0, false);
            if (v > bestNFA) { bestNFA = v; best = r; }
        }
    }
    PSTAT(ST_TNFA, NOW() - t0);
    return bestNFA;
}
