// lsd_grid.hip -- the grid stack's part of the C ABI (include/lsd_hip.h): mapping with known poses (k_gridmap.hip), the correlative
// scan-to-grid match, plain (k_gridmatch.hip) and coarse to fine (k_gridmatch_mr.hip), and the response around a match
// (k_gridresponse.hip), ray casting (k_gridray.hip) and the global localisation (k_gridlocate.hip).  The scan-taking device entries receive the scans of a frame the same way: one check (grid_scans_bad)
// turns those arguments into the view the launchers take, and each entry adds only what is its own.  Their host conveniences share one
// check (host_scans_bad) in the same way, and every host convenience here is one round trip through the context's staging (lsd_ctx.h:
// stage_round_trip).
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "lsd_ctx.h"

// the pose is the first three doubles of each record the entry's pitch may step over
static_assert(sizeof(lsd_position) == 24 && offsetof(lsd_position, x) == 0 && offsetof(lsd_position, y) == 8 && offsetof(lsd_position, ang) == 16 &&
              sizeof(lsd_fa_state) == 720 && offsetof(lsd_fa_state, x) == 0 && offsetof(lsd_fa_carry, state) == 0 && sizeof(lsd_fa_carry) == 768,
              "lsd_enqueue_grid_integrate_device reads a pose from the head of lsd_position, lsd_fa_state and lsd_fa_carry records");

static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// what every entry that takes scans refuses about the sizes, the frame and the range (c not null)
static bool grid_frame_bad(const lsd_ctx* c, int n_scans, int stride, const lsd_map_param& mp, double range_max) {
    if (n_scans < 0 || stride <= 0 || stride > c->scan_cap) return true;
    if (mp.oriMapCol <= 0 || mp.oriMapRow <= 0 || mp.oriMapCol > 65535 || mp.oriMapRow > 65535) return true;
    return !(mp.mapResol > 0) || !(range_max > 0) || !(range_max / mp.mapResol < 32767);     // (a NaN fails every test)
}

// The leading arguments of a scan-taking device entry: refused (true; with c->err naming `entry` where it is the pitch or an alignment),
// or handed on as the view the launchers take.
static bool grid_scans_bad(lsd_ctx* c, const char* entry, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                           size_t pose_pitch, const lsd_map_param& mp, double range_max, GridScans& g) {
    if (!c || !d_scans || !d_lens || !d_poses || grid_frame_bad(c, n_scans, stride, mp, range_max)) return true;
    if (pose_pitch < sizeof(lsd_position) || pose_pitch % 8 || (addr(d_scans) & 15) || (addr(d_poses) & 7)) {
        c->err = std::string(entry) + ": pose pitch >= 24 and a multiple of 8, d_scans 16-byte and d_poses 8-byte aligned";
        return true;
    }
    g = GridScans{d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp.oriMapCol, mp.oriMapRow, mp.mapResol, range_max};
    return false;
}

// ... and those of a host entry, whose lengths can be read: each within 0..stride
static bool host_scans_bad(const lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses,
                           const lsd_map_param& mp, double range_max) {
    if (!c || !scans || !lens || !poses || grid_frame_bad(c, n_scans, stride, mp, range_max)) return true;
    for (int i = 0; i < n_scans; i++) if (lens[i] < 0 || lens[i] > stride) return true;
    return false;
}

extern "C" {

// --- mapping with known poses (k_gridmap.hip) ---
int lsd_enqueue_grid_integrate_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                                      size_t pose_pitch, lsd_map_param mp, double range_max, uint32_t* d_pass, uint32_t* d_hit, void* stream) {
    GridScans g;
    if (!d_pass || !d_hit || grid_scans_bad(c, "grid integrate", d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp, range_max, g))
        return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) { launch_grid_integrate(g, d_pass, d_hit, s); return LSD_OK; });
}

int lsd_enqueue_grid_publish_device(lsd_ctx* c, const uint32_t* d_pass, const uint32_t* d_hit, size_t n_cells, uint32_t min_pass,
                                    uint32_t occ_num, uint32_t occ_den, int8_t* d_grid, void* stream) {
    if (!c || !d_pass || !d_hit || !d_grid || n_cells == 0 || occ_den == 0 || occ_num > occ_den) return LSD_ERR_INVALID;
    if (n_cells > (size_t)65535 * 65535) return LSD_ERR_INVALID;      // (more cells than the largest grid the integration takes)
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_grid_publish(d_pass, d_hit, n_cells, min_pass, occ_num, occ_den, d_grid, s);
        return LSD_OK;
    });
}

int lsd_grid_integrate(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses, lsd_map_param mp,
                       double range_max, uint32_t* pass, uint32_t* hit) {
    if (!pass || !hit || host_scans_bad(c, scans, lens, n_scans, stride, poses, mp, range_max)) return LSD_ERR_INVALID;
    // (no scans: the planes still make the round trip)
    const size_t ns = (size_t)n_scans, cells = (size_t)mp.oriMapCol * mp.oriMapRow;
    lsd_polar* d_sc; int* d_len; lsd_position* d_po; uint32_t *d_pa, *d_hi;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_po, poses, ns); k.both(d_pa, pass, cells); k.both(d_hi, hit, cells);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_grid_integrate_device(c, d_sc, d_len, n_scans, stride, d_po, sizeof(lsd_position), mp, range_max, d_pa, d_hi, c->stream);
    });
}

// --- correlative scan-to-grid matching (k_gridmatch.hip) ---
int lsd_grid_smear_default(double sigma_cells, int radius, lsd_grid_smear* out) {
    if (!out || radius < 0 || radius > 7 || !(sigma_cells > 0) || !std::isfinite(sigma_cells)) return LSD_ERR_INVALID;
    memset(out, 0, sizeof *out);
    out->radius = radius;
    for (int v = 0; v <= radius; v++)
        for (int u = 0; u <= radius; u++) out->w[v][u] = (uint8_t)floor(255 * exp(-(double)(u * u + v * v) / (2 * sigma_cells * sigma_cells)) + 0.5);
    return LSD_OK;
}

int lsd_enqueue_grid_likelihood_device(lsd_ctx* c, const uint32_t* d_pass, const uint32_t* d_hit, int cols, int rows, uint32_t min_pass,
                                       uint32_t occ_num, uint32_t occ_den, lsd_grid_smear smear, uint8_t* d_corr, void* stream) {
    if (!c || !d_pass || !d_hit || !d_corr || cols <= 0 || rows <= 0 || cols > 65535 || rows > 65535) return LSD_ERR_INVALID;
    if (smear.radius < 0 || smear.radius > 7 || occ_den == 0 || occ_num > occ_den) return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_grid_likelihood(d_pass, d_hit, cols, rows, min_pass, occ_num, occ_den, smear, d_corr, s);
        return LSD_OK;
    });
}

// what both match entries refuse about the search
static bool grid_search_bad(const lsd_grid_search& se) {
    if (se.wx < 0 || se.wx > 63 || se.wy < 0 || se.wy > 63 || se.na < 0 || se.na > 63) return true;
    if (!std::isfinite(se.ang_step) || se.ang_step < 0 || (se.ang_step == 0 && se.na > 0)) return true;
    return se.min_den == 0 || se.min_num > se.min_den;
}

int lsd_enqueue_grid_match_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                                  size_t pose_pitch, lsd_map_param mp, double range_max, const uint8_t* d_corr, lsd_grid_search se,
                                  lsd_grid_match_rec* d_out, void* stream) {
    GridScans g;
    if (!d_corr || !d_out || grid_search_bad(se) ||
        grid_scans_bad(c, "grid match", d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp, range_max, g))
        return LSD_ERR_INVALID;
    if (addr(d_out) & 7) {
        c->err = "grid match: d_out 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        HIPCHK(c, c->gm_slots.reserve(grid_match_slot_bytes(n_scans, se.na)));   // (grown: one synchronisation; else nothing happens)
        launch_grid_match(g, d_corr, se, c->gm_slots.get(), d_out, s);
        return LSD_OK;
    });
}

int lsd_grid_match(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses, lsd_map_param mp,
                   double range_max, const uint8_t* corr, lsd_grid_search se, lsd_grid_match_rec* out) {
    if (!corr || !out || grid_search_bad(se) || host_scans_bad(c, scans, lens, n_scans, stride, poses, mp, range_max)) return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    const size_t ns = (size_t)n_scans, cells = (size_t)mp.oriMapCol * mp.oriMapRow;
    lsd_polar* d_sc; int* d_len; lsd_position* d_po; uint8_t* d_co; lsd_grid_match_rec* d_out;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_po, poses, ns); k.in(d_co, corr, cells); k.out(d_out, out, ns);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_grid_match_device(c, d_sc, d_len, n_scans, stride, d_po, sizeof(lsd_position), mp, range_max, d_co, se, d_out, c->stream);
    });
}

// --- the same match, coarse to fine (k_gridmatch_mr.hip) ---
size_t lsd_grid_coarse_bytes(int cols, int rows, int block) {
    if (cols <= 0 || rows <= 0 || cols > 65535 || rows > 65535 || block < 2 || block > 16) return 0;
    return (size_t)(cols + block - 1) * (rows + block - 1);
}

int lsd_enqueue_grid_coarse_device(lsd_ctx* c, const uint8_t* d_corr, int cols, int rows, int block, uint8_t* d_coarse, void* stream) {
    if (!c || !d_corr || !d_coarse || lsd_grid_coarse_bytes(cols, rows, block) == 0) return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) { launch_grid_coarse(d_corr, cols, rows, block, d_coarse, s); return LSD_OK; });
}

int lsd_enqueue_grid_match_mr_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                                     size_t pose_pitch, lsd_map_param mp, double range_max, const uint8_t* d_corr, const uint8_t* d_coarse,
                                     int block, lsd_grid_search se, lsd_grid_match_rec* d_out, lsd_grid_match_mr_stats* d_stats, void* stream) {
    GridScans g;
    if (!d_corr || !d_coarse || !d_out || grid_search_bad(se) || block < 2 || block > 16 ||
        grid_scans_bad(c, "grid match", d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp, range_max, g))
        return LSD_ERR_INVALID;
    if ((addr(d_out) & 7) || (addr(d_stats) & 3)) {
        c->err = "grid match: d_out 8-byte, d_stats 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        size_t bytes[4];
        grid_match_mr_ws(n_scans, se, block, bytes);
        uint8_t* r[4];
        auto regions = [&](Carver& k) { for (int i = 0; i < 4; i++) k(r[i], bytes[i]); };
        HIPCHK(c, carve(c->gm_mr_ws, regions));                      // (grown: one synchronisation; else nothing but pointer arithmetic)
        void* const ws[4] = {r[0], r[1], r[2], r[3]};
        launch_grid_match_mr(g, d_corr, d_coarse, block, se, ws, d_out, d_stats, s);
        return LSD_OK;
    });
}

int lsd_grid_match_mr(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses, lsd_map_param mp,
                      double range_max, const uint8_t* corr, int block, lsd_grid_search se, lsd_grid_match_rec* out, lsd_grid_match_mr_stats* stats) {
    if (!corr || !out || grid_search_bad(se) || block < 2 || block > 16 || host_scans_bad(c, scans, lens, n_scans, stride, poses, mp, range_max))
        return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    const size_t ns = (size_t)n_scans, cells = (size_t)mp.oriMapCol * mp.oriMapRow;
    lsd_polar* d_sc; int* d_len; lsd_position* d_po; uint8_t *d_co, *d_cs; lsd_grid_match_rec* d_out; lsd_grid_match_mr_stats* d_st;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_po, poses, ns);
        k.in(d_co, corr, cells); k.scratch(d_cs, lsd_grid_coarse_bytes(mp.oriMapCol, mp.oriMapRow, block)); k.out(d_out, out, ns); k.out(d_st, stats, ns);
    };
    return stage_round_trip(c, plan, [&] {
        const int st = lsd_enqueue_grid_coarse_device(c, d_co, mp.oriMapCol, mp.oriMapRow, block, d_cs, c->stream);
        if (st != LSD_OK) return st;
        return lsd_enqueue_grid_match_mr_device(c, d_sc, d_len, n_scans, stride, d_po, sizeof(lsd_position), mp, range_max, d_co, d_cs, block, se, d_out,
                                                stats ? d_st : nullptr, c->stream);
    });
}

// --- the response around a match (k_gridresponse.hip) ---
size_t lsd_grid_response_volume_bytes(int n_scans, lsd_grid_response_par rp) {
    if (n_scans < 0 || rp.rx < 1 || rp.rx > 7 || rp.ry < 1 || rp.ry > 7 || rp.ra < 0 || rp.ra > 7) return 0;
    return grid_response_volume_bytes(n_scans, rp);
}

// what both response entries refuse about the window (one scan's volume has no size), the keep ratio and the step
static bool grid_response_bad(const lsd_grid_response_par& rp, double ang_step) {
    if (lsd_grid_response_volume_bytes(1, rp) == 0 || rp.keep_den == 0 || rp.keep_num > rp.keep_den) return true;
    return !std::isfinite(ang_step) || ang_step < 0 || (ang_step == 0 && rp.ra > 0);
}

int lsd_enqueue_grid_response_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                                     size_t pose_pitch, const lsd_grid_match_rec* d_records, lsd_map_param mp, double range_max,
                                     const uint8_t* d_corr, double ang_step, lsd_grid_response_par rp, lsd_grid_response_rec* d_out,
                                     uint32_t* d_volume, void* stream) {
    GridScans g;
    if (!d_records || !d_corr || !d_out || grid_response_bad(rp, ang_step) ||
        grid_scans_bad(c, "grid response", d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp, range_max, g))
        return LSD_ERR_INVALID;
    if (((addr(d_records) | addr(d_out)) & 7) || (addr(d_volume) & 3)) {
        c->err = "grid response: d_records and d_out 8-byte, d_volume 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        if (!d_volume) {
            // (grown: one synchronisation; else nothing happens)
            HIPCHK(c, c->gr_volume.reserve(grid_response_volume_bytes(n_scans, rp) / sizeof(uint32_t)));
            d_volume = c->gr_volume.get();
        }
        launch_grid_response(g, d_records, d_corr, ang_step, rp, d_volume, d_out, s);
        return LSD_OK;
    });
}

int lsd_grid_response(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses,
                      const lsd_grid_match_rec* records, lsd_map_param mp, double range_max, const uint8_t* corr, double ang_step,
                      lsd_grid_response_par rp, lsd_grid_response_rec* out, uint32_t* volume) {
    if (!records || !corr || !out || grid_response_bad(rp, ang_step) || host_scans_bad(c, scans, lens, n_scans, stride, poses, mp, range_max))
        return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    const size_t ns = (size_t)n_scans, cells = (size_t)mp.oriMapCol * mp.oriMapRow, n_vol = grid_response_volume_bytes(n_scans, rp) / sizeof(uint32_t);
    lsd_polar* d_sc; int* d_len; lsd_position* d_po; lsd_grid_match_rec* d_rec; uint8_t* d_co; lsd_grid_response_rec* d_out; uint32_t* d_vol;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_po, poses, ns);
        k.in(d_rec, records, ns); k.in(d_co, corr, cells); k.out(d_out, out, ns); k.out(d_vol, volume, n_vol);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_grid_response_device(c, d_sc, d_len, n_scans, stride, d_po, sizeof(lsd_position), d_rec, mp, range_max, d_co, ang_step, rp, d_out,
                                                d_vol, c->stream);
    });
}

// --- ray casting on the grid (k_gridray.hip) ---
static_assert(sizeof(lsd_grid_ray) == 32 && offsetof(lsd_grid_ray, r_exp) == 0 && offsetof(lsd_grid_ray, r_unk) == 8 && offsetof(lsd_grid_ray, cx) == 16 &&
              offsetof(lsd_grid_ray, cy) == 20 && offsetof(lsd_grid_ray, k_hit) == 24 && offsetof(lsd_grid_ray, cls) == 28,
              "lsd_grid_ray is 32 bytes: two doubles, three int32, the class");
static_assert(sizeof(lsd_grid_ray_sum) == 64 && offsetof(lsd_grid_ray_sum, x) == 0 && offsetof(lsd_grid_ray_sum, y) == 8 &&
              offsetof(lsd_grid_ray_sum, ang) == 16 && offsetof(lsd_grid_ray_sum, n) == 24 && offsetof(lsd_grid_ray_sum, judged) == 52 &&
              offsetof(lsd_grid_ray_sum, flags) == 56 && offsetof(lsd_grid_ray_sum, pad) == 60,
              "lsd_grid_ray_sum is 64 bytes and starts with a pose: an array of them is a d_poses argument of pitch 64");
static_assert(sizeof(lsd_grid_ray_par) == 32 && offsetof(lsd_grid_ray_par, drop_mask) == 8 && offsetof(lsd_grid_ray_par, gate) == 24, "lsd_grid_ray_par");

// what both ray-casting entries refuse about the parameters
static bool grid_ray_bad(const lsd_grid_ray_par& par) {
    if (!std::isfinite(par.tol) || par.tol < 0 || par.drop_mask >= 128) return true;
    return par.ok_den == 0 || par.ok_num > par.ok_den;
}

int lsd_enqueue_grid_raycast_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, const void* d_poses,
                                    size_t pose_pitch, lsd_map_param mp, double range_max, const int8_t* d_grid, lsd_grid_ray_par par,
                                    lsd_grid_ray* d_out, lsd_grid_ray_sum* d_sum, lsd_polar* d_scans_out, void* stream) {
    GridScans g;
    if (!d_grid || !d_out || !d_sum || grid_ray_bad(par) ||
        grid_scans_bad(c, "grid raycast", d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, mp, range_max, g))
        return LSD_ERR_INVALID;
    if (((addr(d_out) | addr(d_sum)) & 7) || (addr(d_scans_out) & 15)) {
        c->err = "grid raycast: d_out and d_sum 8-byte, d_scans_out 16-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (d_scans_out && d_scans_out != d_scans) {                         // in place, or apart
        const uintptr_t bytes = (uintptr_t)n_scans * stride * sizeof(lsd_polar), a = addr(d_scans), b = addr(d_scans_out);
        if (a < b + bytes && b < a + bytes) {
            c->err = "grid raycast: d_scans_out is d_scans itself or does not overlap it";
            return LSD_ERR_INVALID;
        }
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) { launch_grid_raycast(g, d_grid, par, d_out, d_sum, d_scans_out, s); return LSD_OK; });
}

int lsd_grid_raycast(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, const lsd_position* poses, lsd_map_param mp,
                     double range_max, const int8_t* grid, lsd_grid_ray_par par, lsd_grid_ray* out, lsd_grid_ray_sum* sum, lsd_polar* scans_out) {
    if (!grid || !out || !sum || grid_ray_bad(par) || host_scans_bad(c, scans, lens, n_scans, stride, poses, mp, range_max)) return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    const size_t ns = (size_t)n_scans, beams = ns * stride, cells = (size_t)mp.oriMapCol * mp.oriMapRow;
    lsd_polar *d_sc, *d_so; int* d_len; lsd_position* d_po; int8_t* d_gr; lsd_grid_ray* d_out; lsd_grid_ray_sum* d_sum;
    auto plan = [&](StagePass& k) {                                      // (the slots of `out` at i >= len are the caller's: they make the round trip)
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_po, poses, ns);
        k.in(d_gr, grid, cells); k.both(d_out, out, beams); k.out(d_sum, sum, ns); k.both(d_so, scans_out, scans_out ? beams : 0);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_grid_raycast_device(c, d_sc, d_len, n_scans, stride, d_po, sizeof(lsd_position), mp, range_max, d_gr, par, d_out, d_sum,
                                               scans_out ? d_so : nullptr, c->stream);
    });
}

// --- global scan-to-grid localisation (k_gridlocate.hip) ---
static_assert(sizeof(lsd_grid_locate_par) == 64 && offsetof(lsd_grid_locate_par, nx) == 8 && offsetof(lsd_grid_locate_par, ang0) == 16 &&
              offsetof(lsd_grid_locate_par, n_ang) == 32 && offsetof(lsd_grid_locate_par, max_nodes) == 40 && offsetof(lsd_grid_locate_par, min_den) == 56,
              "lsd_grid_locate_par is 64 bytes: four int32, two doubles, two int32, five uint32");
static_assert(sizeof(lsd_grid_locate_rec) == 64 && offsetof(lsd_grid_locate_rec, x) == 0 && offsetof(lsd_grid_locate_rec, y) == 8 &&
              offsetof(lsd_grid_locate_rec, ang) == 16 && offsetof(lsd_grid_locate_rec, reserved) == 56,
              "lsd_grid_locate_rec is 64 bytes and starts with a pose: an array of them is a d_poses argument of pitch 64");

static bool grid_pyramid_bad(int cols, int rows, int levels) {
    return cols <= 0 || rows <= 0 || cols > 65535 || rows > 65535 || levels < 0 || levels > LSD_GRID_LOCATE_MAX_LEVELS;
}

size_t lsd_grid_pyramid_bytes(int cols, int rows, int levels) {
    return grid_pyramid_bad(cols, rows, levels) ? 0 : grid_pyramid_offset(cols, rows, levels + 1);
}

size_t lsd_grid_pyramid_offset(int cols, int rows, int h) {
    return grid_pyramid_bad(cols, rows, h) ? (size_t)-1 : grid_pyramid_offset(cols, rows, h);
}

int lsd_enqueue_grid_pyramid_device(lsd_ctx* c, const uint8_t* d_corr, int cols, int rows, int levels, uint8_t* d_pyramid, void* stream) {
    if (!c || !d_corr || !d_pyramid || grid_pyramid_bad(cols, rows, levels)) return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) { launch_grid_pyramid(d_corr, cols, rows, levels, d_pyramid, s); return LSD_OK; });
}

// what the locate entries refuse about the box, the headings, the levels and the acceptance
static bool grid_locate_bad(const lsd_grid_locate_par& p) {
    if (p.x0 < -(1 << 20) || p.x0 > (1 << 20) || p.y0 < -(1 << 20) || p.y0 > (1 << 20)) return true;
    if (p.nx < 1 || p.nx > 65535 || p.ny < 1 || p.ny > 65535 || p.n_ang < 1 || p.n_ang > 4096) return true;
    if (!std::isfinite(p.ang0) || !std::isfinite(p.ang_step) || p.ang_step < 0 || (p.ang_step == 0 && p.n_ang > 1)) return true;
    if (p.levels < 0 || p.levels > LSD_GRID_LOCATE_MAX_LEVELS || p.max_nodes < 1 || p.max_nodes > (1u << 24)) return true;
    if (p.min_den == 0 || p.min_num > p.min_den) return true;
    return grid_locate_top_nodes(p) > ((size_t)1 << 28);
}

size_t lsd_grid_locate_workspace_bytes(int n_scans, int stride, lsd_grid_locate_par par) {
    if (n_scans < 0 || stride <= 0 || stride > LSD_SCAN_MAX_LEN || grid_locate_bad(par)) return 0;
    size_t bytes[kGridLocateRegions];
    grid_locate_ws(n_scans, stride, par, bytes);
    Carver measure(nullptr);
    uint8_t* r;
    for (int i = 0; i < kGridLocateRegions; i++) measure(r, bytes[i]);
    return measure.bytes_from(nullptr);
}

int lsd_enqueue_grid_locate_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, lsd_map_param mp,
                                   double range_max, const uint8_t* d_pyramid, lsd_grid_locate_par par, lsd_grid_locate_rec* d_out,
                                   lsd_grid_locate_stats* d_stats, void* stream) {
    if (!c || !d_scans || !d_lens || !d_pyramid || !d_out || grid_frame_bad(c, n_scans, stride, mp, range_max) || grid_locate_bad(par))
        return LSD_ERR_INVALID;
    if ((addr(d_scans) & 15) || (addr(d_lens) & 3) || (addr(d_out) & 7) || (addr(d_stats) & 3)) {
        c->err = "grid locate: d_scans 16-byte, d_out 8-byte, d_lens and d_stats 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        size_t bytes[kGridLocateRegions];
        grid_locate_ws(n_scans, stride, par, bytes);
        uint8_t* r[kGridLocateRegions];
        auto regions = [&](Carver& k) { for (int i = 0; i < kGridLocateRegions; i++) k(r[i], bytes[i]); };
        HIPCHK(c, carve(c->gl_ws, regions));                         // (grown: one synchronisation; else nothing but pointer arithmetic)
        void* ws[kGridLocateRegions];
        for (int i = 0; i < kGridLocateRegions; i++) ws[i] = r[i];
        launch_grid_locate(d_scans, d_lens, n_scans, stride, mp.oriMapCol, mp.oriMapRow, mp.mapResol, range_max, d_pyramid, par, ws, d_out, d_stats, s);
        return LSD_OK;
    });
}

// the host convenience of both locate entries: the uploads, the pyramid, `enqueue` on the staged arrays, the read-back of the records and
// of stats_bytes per scan
extern "C++" {
template <class Enqueue>
static int grid_locate_host(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, lsd_map_param mp, double range_max,
                            const uint8_t* corr, lsd_grid_locate_par par, lsd_grid_locate_rec* out, void* stats, size_t stats_bytes, Enqueue enqueue) {
    if (!c || !scans || !lens || !corr || !out || grid_frame_bad(c, n_scans, stride, mp, range_max) || grid_locate_bad(par)) return LSD_ERR_INVALID;
    for (int i = 0; i < n_scans; i++) if (lens[i] < 0 || lens[i] > stride) return LSD_ERR_INVALID;
    if (n_scans == 0) return LSD_OK;
    const size_t ns = (size_t)n_scans, cells = (size_t)mp.oriMapCol * mp.oriMapRow;
    lsd_polar* d_sc; int* d_len; uint8_t *d_co, *d_py; lsd_grid_locate_rec* d_out; uint64_t* d_st;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.in(d_co, corr, cells);
        k.scratch(d_py, lsd_grid_pyramid_bytes(mp.oriMapCol, mp.oriMapRow, par.levels)); k.out(d_out, out, ns);
        k.out(d_st, static_cast<uint64_t*>(stats), ns * stats_bytes / sizeof(uint64_t));
    };
    return stage_round_trip(c, plan, [&] {
        const int st = lsd_enqueue_grid_pyramid_device(c, d_co, mp.oriMapCol, mp.oriMapRow, par.levels, d_py, c->stream);
        return st != LSD_OK ? st : enqueue(d_sc, d_len, d_py, d_out, stats ? d_st : nullptr);
    });
}
}  // extern "C++"

int lsd_grid_locate(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, lsd_map_param mp, double range_max,
                    const uint8_t* corr, lsd_grid_locate_par par, lsd_grid_locate_rec* out, lsd_grid_locate_stats* stats) {
    return grid_locate_host(c, scans, lens, n_scans, stride, mp, range_max, corr, par, out, stats, sizeof(lsd_grid_locate_stats),
                            [&](lsd_polar* d_sc, int* d_len, uint8_t* d_py, lsd_grid_locate_rec* d_out, uint64_t* d_st) {
                                return lsd_enqueue_grid_locate_device(c, d_sc, d_len, n_scans, stride, mp, range_max, d_py, par, d_out,
                                                                      reinterpret_cast<lsd_grid_locate_stats*>(d_st), c->stream);
                            });
}

// --- the tight search (k_gridlocate_tight.hip) ---
static_assert(sizeof(lsd_grid_locate_tight_stats) == 128 && sizeof(lsd_grid_locate_stats) % 8 == 0, "the statistics records, staged as 64-bit words");

static bool grid_locate_tight_bad(uint32_t tight) { return (tight & ~(LSD_GRID_LOCATE_TIGHT_PROBE | LSD_GRID_LOCATE_TIGHT_RETRY)) != 0; }

size_t lsd_grid_locate_tight_workspace_bytes(int n_scans, int stride, lsd_grid_locate_par par) {
    if (n_scans < 0 || stride <= 0 || stride > LSD_SCAN_MAX_LEN || grid_locate_bad(par)) return 0;
    size_t bytes[kGridLocateTightRegions];
    grid_locate_tight_ws(n_scans, stride, par, bytes);
    Carver measure(nullptr);
    uint8_t* r;
    for (int i = 0; i < kGridLocateTightRegions; i++) measure(r, bytes[i]);
    return measure.bytes_from(nullptr);
}

int lsd_enqueue_grid_locate_tight_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, lsd_map_param mp,
                                         double range_max, const uint8_t* d_pyramid, lsd_grid_locate_par par, uint32_t tight,
                                         lsd_grid_locate_rec* d_out, lsd_grid_locate_tight_stats* d_stats, void* stream) {
    if (!c || !d_scans || !d_lens || !d_pyramid || !d_out || grid_frame_bad(c, n_scans, stride, mp, range_max) || grid_locate_bad(par))
        return LSD_ERR_INVALID;
    if (grid_locate_tight_bad(tight)) {
        c->err = "grid locate: tight is LSD_GRID_LOCATE_TIGHT_PROBE | LSD_GRID_LOCATE_TIGHT_RETRY at the most";
        return LSD_ERR_INVALID;
    }
    if ((addr(d_scans) & 15) || (addr(d_lens) & 3) || (addr(d_out) & 7) || (addr(d_stats) & 3)) {
        c->err = "grid locate: d_scans 16-byte, d_out 8-byte, d_lens and d_stats 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_scans == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        size_t bytes[kGridLocateTightRegions];
        grid_locate_tight_ws(n_scans, stride, par, bytes);
        uint8_t* r[kGridLocateTightRegions];
        auto regions = [&](Carver& k) { for (int i = 0; i < kGridLocateTightRegions; i++) k(r[i], bytes[i]); };
        HIPCHK(c, carve(c->gl_ws, regions));                         // (grown: one synchronisation; else nothing but pointer arithmetic)
        void* ws[kGridLocateTightRegions];
        for (int i = 0; i < kGridLocateTightRegions; i++) ws[i] = r[i];
        launch_grid_locate_tight(d_scans, d_lens, n_scans, stride, mp.oriMapCol, mp.oriMapRow, mp.mapResol, range_max, d_pyramid, par, tight, ws, d_out,
                                 d_stats, s);
        return LSD_OK;
    });
}

int lsd_grid_locate_tight(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, lsd_map_param mp, double range_max,
                          const uint8_t* corr, lsd_grid_locate_par par, uint32_t tight, lsd_grid_locate_rec* out, lsd_grid_locate_tight_stats* stats) {
    if (grid_locate_tight_bad(tight)) return LSD_ERR_INVALID;
    return grid_locate_host(c, scans, lens, n_scans, stride, mp, range_max, corr, par, out, stats, sizeof(lsd_grid_locate_tight_stats),
                            [&](lsd_polar* d_sc, int* d_len, uint8_t* d_py, lsd_grid_locate_rec* d_out, uint64_t* d_st) {
                                return lsd_enqueue_grid_locate_tight_device(c, d_sc, d_len, n_scans, stride, mp, range_max, d_py, par, tight, d_out,
                                                                            reinterpret_cast<lsd_grid_locate_tight_stats*>(d_st), c->stream);
                            });
}

}  // extern "C"
