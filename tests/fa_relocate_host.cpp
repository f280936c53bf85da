// fa_relocate_host.cpp -- test program (tests/test_fa_relocate_cpu.py): the part of the relocalisation's host side that needs no GPU
// (csrc/fa_relocate_host.h: the argument checks of lsd_enqueue_fa_lost_gather_device and lsd_enqueue_fa_carry_seed_device, the element
// counts of lsd_fa_lost_gather's staging) driven under the host sanitizers, with the regions laid out by the host side's own carver
// (csrc/lsd_devbuf.h) in HOST memory and written from end to end, so that a count that is too small or wraps shows as an overflow.
// Built with -fsanitize=address,undefined; exits 0 and prints "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "fa_relocate_host.h"
#include "lsd_devbuf.h"

using namespace lsdhip;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

struct LostArgs {
    bool ctx = true; int cap = 1024; const void* carry; int n_seq = 3; int fp = 2; const void* poses; size_t pitch = 720; const void* scans;
    const void* lens; int stride = 360; const void* key = nullptr; int max_lost = 2; const void* scans_out; const void* lens_out; const void* pick;
    const void* n_lost;
    bool refused() const {
        return fa_lost_refused(ctx, cap, carry, n_seq, fp, poses, pitch, scans, lens, stride, key, max_lost, scans_out, lens_out, pick, n_lost);
    }
};

struct SeedArgs {
    bool ctx = true; const void* carry; int n_seq = 3; int fp = 2; const void* pick; int n_pick = 2; const void* loc; const void* resp = nullptr;
    lsd_fa_seed_par par{1.0, 1.0, 1.0, 1.0, 1.0, 1u, 0u}; const void* rep = nullptr;
    bool refused() const { return fa_seed_refused(ctx, carry, n_seq, fp, pick, n_pick, loc, resp, par, rep); }
};

int main() {
    alignas(64) static unsigned char mem[256];
    const void* a = mem;                                            // aligned to 64
    auto at = [](int off) -> const void* { return mem + off; };
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the gather's refusals: the base call is taken, every single departure is refused
    LostArgs g;
    g.carry = g.poses = g.scans = g.lens = g.scans_out = g.lens_out = g.pick = g.n_lost = a;
    EXPECT(!g.refused());
    { LostArgs b = g; b.key = at(4); EXPECT(!b.refused()); b.key = at(2); EXPECT(b.refused()); }
    { LostArgs b = g; b.ctx = false; EXPECT(b.refused()); }
    const void* LostArgs::*ptrs[] = {&LostArgs::carry, &LostArgs::poses, &LostArgs::scans, &LostArgs::lens, &LostArgs::scans_out, &LostArgs::lens_out,
                                     &LostArgs::pick, &LostArgs::n_lost};
    for (auto p : ptrs) { LostArgs b = g; b.*p = nullptr; EXPECT(b.refused()); }
    for (int v : {0, -1, 65537}) { LostArgs b = g; b.n_seq = v; EXPECT(b.refused()); }
    for (int v : {1, 65536}) { LostArgs b = g; b.n_seq = v; EXPECT(!b.refused()); }
    for (int v : {0, -5, 4097}) { LostArgs b = g; b.fp = v; EXPECT(b.refused()); }
    for (int v : {1, 4096}) { LostArgs b = g; b.fp = v; EXPECT(!b.refused()); }
    for (size_t v : {(size_t)0, (size_t)16, (size_t)23, (size_t)28, (size_t)721}) { LostArgs b = g; b.pitch = v; EXPECT(b.refused()); }
    for (size_t v : {(size_t)24, (size_t)64, (size_t)192}) { LostArgs b = g; b.pitch = v; EXPECT(!b.refused()); }
    for (int v : {0, -1, 1025}) { LostArgs b = g; b.stride = v; EXPECT(b.refused()); }
    { LostArgs b = g; b.stride = 1025; b.cap = 4096; EXPECT(!b.refused()); b.stride = 4097; EXPECT(b.refused()); }
    for (int v : {0, -1, 4097}) { LostArgs b = g; b.max_lost = v; EXPECT(b.refused()); }
    for (int v : {1, 4096}) { LostArgs b = g; b.max_lost = v; EXPECT(!b.refused()); }
    { LostArgs b = g; b.carry = at(4); EXPECT(b.refused()); b.carry = at(8); EXPECT(!b.refused()); }
    { LostArgs b = g; b.poses = at(4); EXPECT(b.refused()); b.poses = at(8); EXPECT(!b.refused()); }
    { LostArgs b = g; b.scans = at(8); EXPECT(b.refused()); b.scans = at(16); EXPECT(!b.refused()); }
    { LostArgs b = g; b.scans_out = at(8); EXPECT(b.refused()); b.scans_out = at(32); EXPECT(!b.refused()); }
    for (auto p : {&LostArgs::lens, &LostArgs::lens_out, &LostArgs::pick, &LostArgs::n_lost}) {
        LostArgs b = g; b.*p = at(2); EXPECT(b.refused()); b.*p = at(1); EXPECT(b.refused()); b.*p = at(4); EXPECT(!b.refused());
    }

    // ---- the seed's refusals
    SeedArgs s;
    s.carry = s.pick = s.loc = a;
    EXPECT(!s.refused());
    { SeedArgs b = s; b.ctx = false; EXPECT(b.refused()); }
    for (auto p : {&SeedArgs::carry, &SeedArgs::pick, &SeedArgs::loc}) { SeedArgs b = s; b.*p = nullptr; EXPECT(b.refused()); }
    { SeedArgs b = s; b.resp = a; b.rep = a; EXPECT(!b.refused()); b.resp = at(4); EXPECT(b.refused()); b.resp = a; b.rep = at(4); EXPECT(b.refused()); }
    { SeedArgs b = s; b.carry = at(4); EXPECT(b.refused()); b.carry = a; b.loc = at(4); EXPECT(b.refused()); b.loc = a; b.pick = at(2); EXPECT(b.refused());
      b.pick = at(4); EXPECT(!b.refused()); }
    for (int v : {0, -1}) { SeedArgs b = s; b.n_seq = v; EXPECT(b.refused()); }
    for (int v : {0, 4097}) { SeedArgs b = s; b.fp = v; EXPECT(b.refused()); }
    for (int v : {0, -1, 4097}) { SeedArgs b = s; b.n_pick = v; EXPECT(b.refused()); }
    for (int v : {1, 4096}) { SeedArgs b = s; b.n_pick = v; EXPECT(!b.refused()); }
    { SeedArgs b = s; b.par.max_best = 0; EXPECT(b.refused()); b.par.max_best = 0xFFFFFFFFu; EXPECT(!b.refused()); }
    double lsd_fa_seed_par::*reals[] = {&lsd_fa_seed_par::var_xy, &lsd_fa_seed_par::var_ang, &lsd_fa_seed_par::cov_scale, &lsd_fa_seed_par::floor_xy,
                                        &lsd_fa_seed_par::floor_ang};
    for (auto f : reals)
        for (double v : {-1.0, inf, -inf, nan}) {
            SeedArgs b = s; b.par.*f = v; EXPECT(b.refused());
            b.resp = a; EXPECT(b.refused());
        }
    for (auto f : {&lsd_fa_seed_par::var_xy, &lsd_fa_seed_par::var_ang}) {      // a zero variance: refused only where it is used
        SeedArgs b = s; b.par.*f = 0.0; EXPECT(b.refused());
        b.resp = a; EXPECT(!b.refused());
    }
    for (auto f : {&lsd_fa_seed_par::cov_scale, &lsd_fa_seed_par::floor_xy, &lsd_fa_seed_par::floor_ang}) {
        SeedArgs b = s; b.par.*f = 0.0; EXPECT(!b.refused());
    }

    // ---- the host conveniences' stand-ins: null stays null, a misaligned host pointer passes both checks
    EXPECT(fa_host_stand_in(nullptr) == nullptr && fa_host_stand_in(at(1)) != nullptr && !fa_misaligned(fa_host_stand_in(at(1)), 16));
    { SeedArgs b = s; b.carry = fa_host_stand_in(at(3)); b.pick = fa_host_stand_in(at(1)); b.loc = fa_host_stand_in(at(5)); b.resp = fa_host_stand_in(at(7));
      b.rep = fa_host_stand_in(at(9)); EXPECT(!b.refused()); b.pick = fa_host_stand_in(nullptr); EXPECT(b.refused()); }
    { LostArgs b = g; b.scans = fa_host_stand_in(at(8)); b.lens = fa_host_stand_in(at(1)); EXPECT(!b.refused()); b.scans = fa_host_stand_in(nullptr);
      EXPECT(b.refused()); }

    // ---- the staging arithmetic of lsd_fa_lost_gather
    const FaLostStage big = fa_lost_stage(65536, 4096, 4096, 4096);          // 2^40 readings: no int arithmetic reaches it
    EXPECT(big.carries == 65536u && big.slots == (size_t)1 << 28 && big.readings == (size_t)1 << 40 && big.rows == 4096u &&
           big.readings_out == (size_t)1 << 24);
    const int shapes[][4] = {{1, 1, 1, 1}, {3, 2, 360, 2}, {65, 91, 7, 4}, {1025, 1, 1, 4096}, {2, 181, 1025, 3}};
    for (const auto& sh : shapes) {
        const FaLostStage n = fa_lost_stage(sh[0], sh[1], sh[2], sh[3]);
        EXPECT(n.slots == (size_t)sh[0] * sh[1] && n.readings == n.slots * sh[2] && n.readings_out == (size_t)sh[3] * sh[2]);
        lsd_fa_carry* cy; lsd_position* po; lsd_polar *sc, *so; int *ln, *lo; int32_t *pk, *nl;
        auto regions = [&](Carver& k) { k(cy, n.carries); k(po, n.slots); k(sc, n.readings); k(ln, n.slots); k(so, n.readings_out); k(lo, n.rows);
                                        k(pk, n.rows); k(nl, 2); };
        Carver measure(nullptr);
        regions(measure);
        const size_t bytes = measure.bytes_from(nullptr);
        uint8_t* base = static_cast<uint8_t*>(std::aligned_alloc(256, bytes));
        EXPECT(base != nullptr);
        if (!base) break;
        Carver place(base);
        regions(place);
        EXPECT(place.bytes_from(base) == bytes);
        // what the copies of the host convenience write and read, region by region
        std::memset(cy, 1, n.carries * sizeof(lsd_fa_carry));
        std::memset(po, 2, n.slots * sizeof(lsd_position));
        std::memset(sc, 3, n.readings * sizeof(lsd_polar));
        std::memset(ln, 0, n.slots * sizeof(int));
        std::memset(so, 5, n.readings_out * sizeof(lsd_polar));
        std::memset(lo, 6, n.rows * sizeof(int));
        std::memset(pk, 7, n.rows * sizeof(int32_t));
        std::memset(nl, 8, 2 * sizeof(int32_t));
        EXPECT(reinterpret_cast<uintptr_t>(sc) % 16 == 0 && reinterpret_cast<uintptr_t>(so) % 16 == 0 && reinterpret_cast<uintptr_t>(cy) % 8 == 0);
        EXPECT(reinterpret_cast<uint8_t*>(cy)[0] == 1 && reinterpret_cast<uint8_t*>(sc)[n.readings * sizeof(lsd_polar) - 1] == 3 &&
               reinterpret_cast<uint8_t*>(nl)[7] == 8);
        EXPECT(fa_lost_bad_len(ln, n.slots, sh[2]) == -1);
        ln[n.slots - 1] = sh[2] + 1;
        EXPECT(fa_lost_bad_len(ln, n.slots, sh[2]) == (long long)n.slots - 1);
        ln[n.slots - 1] = sh[2]; ln[0] = -1;
        EXPECT(fa_lost_bad_len(ln, n.slots, sh[2]) == 0);
        std::free(base);
    }
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
