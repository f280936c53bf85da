// lsd_loc.hip -- localisation's part of the C ABI (include/lsd_hip.h): scan-to-map matching (k_match.hip), FeatureScan and the two ingest
// entries (k_rdp.hip, k_rdp_long.hip, k_ingest.hip), FeatureAssociation (k_fa.hip), the operations on the carries -- re-base, correction,
// the gather of the lost and the seed (k_fa.hip, k_facorrect.hip, k_falost.hip, k_faseed.hip) -- and the replay loop's six device entries
// with lsd_localize.  Every enqueue entry is its argument check and then enqueue_on; every host convenience is its own checks around one
// stage_round_trip (lsd_ctx.h).  What the entries share is said once: the FeatureScan entries' body (enqueue_feature_scan), the fleet
// entries' table (map_table_check, map_table_upload), the loop's map and frames (FaLoopMap, FaLoopFrames, fa_enqueue_loop).
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lsd_ctx.h"
#include "fa_relocate_host.h"

static_assert(LSD_SCAN_MAX_LEN == kRdpLongMaxLen, "the header's limit is the long kernel's");
static_assert(sizeof(lsd_map_ref) == 64 && offsetof(lsd_map_ref, d_map_cache) == 0 && offsetof(lsd_map_ref, d_map_lines) == 8 &&
              offsetof(lsd_map_ref, d_n_map) == 16 && offsetof(lsd_map_ref, cols) == 24 && offsetof(lsd_map_ref, rows) == 28 &&
              offsetof(lsd_map_ref, n_map) == 32 && offsetof(lsd_map_ref, mapResol) == 40 && offsetof(lsd_map_ref, mapOriX) == 48 &&
              offsetof(lsd_map_ref, mapOriY) == 56,
              "lsd_map_ref has the layout the Python mirror (MAP_REF_DTYPE) assumes");
static_assert(sizeof(lsd_fa_carry) == 768 && offsetof(lsd_fa_carry, odom) == 720 && offsetof(lsd_fa_carry, ang_sum) == 744 &&
              offsetof(lsd_fa_carry, ang_count) == 752 && offsetof(lsd_fa_carry, frames) == 760 && offsetof(lsd_fa_carry, is_offset) == 764,
              "lsd_fa_carry is plain bytes with the layout the Python mirror (FA_CARRY_DTYPE) assumes");

// The fleet entries' table, checked field by field on the host (nothing the kernels follow is left to the device); *max_n_map: the
// largest n_map, what the loops size their workspace from.
static int map_table_check(const lsd_map_ref* maps, int n_maps, const int32_t* d_map_of, int* max_n_map) {
    if (!maps || n_maps <= 0 || !d_map_of) return LSD_ERR_INVALID;
    if (n_maps > LSD_MAX_MAPS) return LSD_ERR_UNSUPPORTED;
    int mx = 0;
    for (int i = 0; i < n_maps; i++) {
        const lsd_map_ref& m = maps[i];
        if (!m.d_map_cache || m.cols <= 0 || m.rows <= 0 || m.n_map < 0 || (m.n_map > 0 && !m.d_map_lines) || !(m.mapResol > 0))
            return LSD_ERR_INVALID;
        mx = std::max(mx, m.n_map);
    }
    if (max_n_map) *max_n_map = mx;
    return LSD_OK;
}

// The checked table to the device, asynchronously on `s`, the way n_frames travels: a host copy the context owns is the upload's source,
// so the caller's array is free when the entry returns.  half 0: FeatureScan's records, 1: the loops'.
static int map_table_upload(lsd_ctx* c, int half, const lsd_map_ref* maps, int n_maps, hipStream_t s, const lsd_map_ref** d_tab) {
    HIPCHK(c, c->map_tab.reserve(2 * LSD_MAX_MAPS));             // (the first fleet call of a context: one synchronisation)
    lsd_map_ref* h = c->map_tab_host.data() + (size_t)half * LSD_MAX_MAPS;
    lsd_map_ref* d = c->map_tab.get() + (size_t)half * LSD_MAX_MAPS;
    std::copy(maps, maps + n_maps, h);
    HIPCHK(c, hipMemcpyAsync(d, h, sizeof(lsd_map_ref) * (size_t)n_maps, hipMemcpyHostToDevice, s));
    *d_tab = d;
    return LSD_OK;
}

// Before a FeatureScan launch: a stride above 1024 goes to the long kernels (k_rdp_long.hip), whose dynamic LDS at this context's capacity
// may be above the 64 KiB a kernel gets without asking.  Their limit is raised once per context (and again after the capacity changes),
// to the capacity's need: every stride the entries let through fits.
static hipError_t rdp_long_prepare(lsd_ctx* c, int stride) {
    if (stride <= kRdpShortMaxLen || c->rdp_long_ready) return hipSuccess;
    const hipError_t e = prepare_rdp_long(rdp_long_lds(c->scan_cap));
    if (e == hipSuccess) c->rdp_long_ready = true;
    return e;
}

// The two FeatureScan enqueue entries.  What `a` brings tells them apart: one map's frame, or -- a.maps, the HOST table -- the fleet's
// arguments, checked here and the table uploaded in the place of a.maps.
static int enqueue_feature_scan(lsd_ctx* c, RdpScans a, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride, int region_point_limit,
                                double thre_line, double line_dist_thre_m, lsd_line* d_lines_out, int* d_n_lines, lsd_position* d_pts_out, int pts_cap,
                                int* d_n_pts, double* d_lidar_pos, int* d_im_size, void* stream) {
    if (!c || !d_scans || !d_lens || n_scans <= 0 || stride <= 0 || !d_lines_out || !d_n_lines || !d_n_pts || !d_lidar_pos || !d_im_size ||
        pts_cap < 0 || (pts_cap > 0 && !d_pts_out) || (a.maps ? a.scans_per_seq <= 0 : !(a.mapResol > 0)))
        return LSD_ERR_INVALID;
    const lsd_map_ref* maps = a.maps;
    if (maps) {
        const int r = map_table_check(maps, a.n_maps, a.map_of, nullptr);
        if (r != LSD_OK) return r;
    }
    if (stride > c->scan_cap) return LSD_ERR_UNSUPPORTED;
    return enqueue_on(c, stream, [&](hipStream_t s) -> int {         // (s NULL: the default stream, as everywhere in HIP)
        HIPCHK(c, rdp_long_prepare(c, stride));
        if (maps) {
            const int u = map_table_upload(c, 0, maps, a.n_maps, s, &a.maps);
            if (u != LSD_OK) return u;
        }
        a.scans = reinterpret_cast<const double*>(d_scans); a.lens = d_lens; a.n = n_scans; a.stride = stride;
        a.region_point_limit = region_point_limit; a.thre_line = thre_line; a.line_dist_thre_m = line_dist_thre_m;
        RdpOut o{};
        o.lines = d_lines_out; o.n_lines = d_n_lines; o.pts = reinterpret_cast<double*>(d_pts_out); o.pts_cap = pts_cap;
        o.n_pts = d_n_pts; o.lidar_pos = d_lidar_pos; o.im_size = d_im_size;
        launch_rdp(a, o, s);
        return LSD_OK;
    });
}

// the two ingest entries: the checks they share, then one launch of k_ingest
static int enqueue_ingest(lsd_ctx* c, const lsd_polar* d_raw, const float* d_ranges, const float* d_min_inc, int n_scans, int n_beams,
                          const int* d_take, lsd_polar* d_scans, int* d_lens, int stride, void* stream) {
    if (!c || n_scans <= 0 || n_beams <= 0 || stride <= 0 || !d_scans || !d_lens || n_beams > stride) return LSD_ERR_INVALID;
    if (stride > c->scan_cap) return LSD_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(d_raw) | reinterpret_cast<uintptr_t>(d_scans)) & 15) {        // the kernel moves a pair in one 16-byte access
        c->err = "scan ingest: d_raw and d_scans must be 16-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_ingest(d_raw, d_ranges, d_min_inc, n_scans, n_beams, d_take, d_scans, d_lens, stride, s);
        return LSD_OK;
    });
}

// --- device FeatureAssociation (k_fa.hip) ------------------------------------------------------------------------------
// Carves the per-sequence workspace of n_seq sequences with pair_cap pairs each out of c->fa_buf (grown with one synchronisation; while
// it is large enough this is pointer arithmetic only: Localizer.step_device never waits for the device).
static int fa_workspace(lsd_ctx* c, int n_seq, int pair_cap, FaArgs& a) {
    const size_t ns = (size_t)n_seq, pc = (size_t)pair_cap;
    auto regions = [&](Carver& k) {
        k(a.pairs, ns * pc * 2); k(a.n_pairs, ns); k(a.n_cand, ns); k(a.n_frames, ns);
        k(a.cand, ns * pc * 16); k(a.scratch, ns * pc * 8); k(a.ctl, ns * kFaCtl); k(a.aux, ns * kFaAux);
    };
    HIPCHK(c, carve(c->fa_buf, regions));
    a.pair_cap = pair_cap;
    a.lds_bound = c->fa_lds_bound;
    return LSD_OK;
}

// The grid match response fused into the carries (k_facorrect.hip): the argument check of both entries.
static bool fa_correct_refused(const lsd_ctx* c, const void* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch,
                               const void* resp, const void* key, const lsd_fa_correct_par& par, const void* rep) {
    auto off8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; };
    auto bad = [](double v) { return !std::isfinite(v) || v < 0; };
    return !c || !carry || !poses || !resp || n_seq <= 0 || frames_pitch < 1 || frames_pitch > 4096 || pose_pitch < 24 || pose_pitch % 8 != 0 ||
           off8(carry) || off8(poses) || off8(resp) || off8(rep) || (reinterpret_cast<uintptr_t>(key) & 3) != 0 || bad(par.cov_scale) ||
           bad(par.floor_xy) || bad(par.floor_ang) || bad(par.gate);
}

// What the replay loop runs against.  One map: its fields; with d_n_map (the live-map entries) the map's line count is read on the device
// and n_map is its capacity.  Or the table (the *_maps entries; a non-null `maps` is what selects it): sequence s runs against
// maps[d_map_of[s]] and the single-map fields are unused.  Everything the host sizes is sized from n_map, resp. the table's largest.
struct FaLoopMap {
    const double* d_map_cache; int cols, rows; const lsd_line* d_map_lines; int n_map; const int32_t* d_n_map; double map_resol;
    const lsd_map_ref* maps; int n_maps; const int32_t* d_map_of;
};

// The frames of the loop: FeatureScan's outputs, the odometry, where each sequence starts from -- d_init (lsd_enqueue_localize_device,
// odometry n_seq x (frames_pitch + 1)) or d_carry (lsd_enqueue_localize_resume_device, odometry n_seq x frames_pitch), exactly one of
// them -- and the outputs.
struct FaLoopFrames {
    int n_seq, frames_pitch; const int* n_frames;
    const lsd_line* d_lines; const int* d_n_lines; const lsd_position* d_pts; int pts_cap; const int* d_n_pts; const double* d_lidar_pos;
    const lsd_position* d_odom; const lsd_fa_state* d_init; lsd_fa_carry* d_carry; lsd_fa_state* d_states; lsd_fa_report* d_reports;
};

// ... as the six entries receive them, in their order
static FaLoopFrames fa_frames(int n_seq, int frames_pitch, const int* n_frames, const lsd_line* d_lines, const int* d_n_lines, const lsd_position* d_pts,
                              int pts_cap, const int* d_n_pts, const double* d_lidar_pos, const lsd_position* d_odom, const lsd_fa_state* d_init,
                              lsd_fa_carry* d_carry, lsd_fa_state* d_states, lsd_fa_report* d_reports) {
    return {n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, d_init, d_carry, d_states, d_reports};
}

// The replay loop of every device entry point.
static int fa_enqueue_loop(lsd_ctx* c, const FaLoopMap& m, const FaLoopFrames& f, void* stream) {
    const int n_seq = f.n_seq;
    if (!c || n_seq <= 0 || f.frames_pitch <= 0 || !f.n_frames || !f.d_lines || !f.d_n_lines || f.pts_cap < 0 || (f.pts_cap > 0 && !f.d_pts) ||
        !f.d_n_pts || !f.d_lidar_pos || !f.d_odom || !(f.d_init || f.d_carry) || !f.d_states || !f.d_reports)
        return LSD_ERR_INVALID;
    if (!m.maps && (!m.d_map_cache || m.cols <= 0 || m.rows <= 0 || m.n_map < 0 || (m.n_map > 0 && !m.d_map_lines) || !(m.map_resol > 0)))
        return LSD_ERR_INVALID;
    int max_frames = 0;
    for (int i = 0; i < n_seq; i++) {
        if (f.n_frames[i] < 0 || f.n_frames[i] > f.frames_pitch) return LSD_ERR_INVALID;
        max_frames = std::max(max_frames, f.n_frames[i]);
    }
    int n_map = m.n_map;
    if (m.maps) {
        const int r = map_table_check(m.maps, m.n_maps, m.d_map_of, &n_map);
        if (r != LSD_OK) return r;
    }
    if ((long long)n_map * LSD_RDP_MAX_LINES > (1 << 26)) return LSD_ERR_UNSUPPORTED;
    return enqueue_on(c, stream, [&](hipStream_t s) -> int {
        FaArgs a{};
        const int r = fa_workspace(c, n_seq, std::max(1, n_map * LSD_RDP_MAX_LINES), a);
        if (r != LSD_OK) return r;
        c->fa_nf.assign(f.n_frames, f.n_frames + n_seq);
        HIPCHK(c, hipMemcpyAsync(const_cast<int*>(a.n_frames), c->fa_nf.data(), sizeof(int) * (size_t)n_seq, hipMemcpyHostToDevice, s));
        if (m.maps) {
            const int u = map_table_upload(c, 1, m.maps, m.n_maps, s, &a.maps);
            if (u != LSD_OK) return u;
            a.map_of = m.d_map_of; a.n_maps = m.n_maps;
        }
        a.map_cache = m.d_map_cache; a.cols = m.cols; a.rows = m.rows; a.map_lines = m.d_map_lines; a.n_map = n_map; a.d_n_map = m.d_n_map;
        a.scan_lines = f.d_lines; a.n_lines = f.d_n_lines; a.line_pitch = LSD_RDP_MAX_LINES;
        a.pts = reinterpret_cast<const double*>(f.d_pts); a.n_pts = f.d_n_pts; a.pts_pitch = f.pts_cap;
        a.lidar_pos = f.d_lidar_pos; a.frames_pitch = f.frames_pitch; a.odom = f.d_odom; a.given = nullptr;
        a.map_resol = m.maps ? 1.0 : m.map_resol;                    // (the table carries each map's own)
        a.init = f.d_init; a.carry = f.d_carry; a.state_in = nullptr; a.states = f.d_states; a.reports = f.d_reports;
        for (int t = 0; t < max_frames; t++) {
            a.t = t;
            launch_fa_frame(a, n_seq, true, s);
        }
        return LSD_OK;
    });
}

extern "C" {

// --- scan-to-map matching (k_match.hip) ---
int lsd_enqueue_scan_to_map_match_device(lsd_ctx* c, const double* d_map_cache, int cols, int rows, const lsd_line* d_map_lines,
                                         const lsd_line* d_scan_lines, const lsd_position* d_pts, int n_points,
                                         lsd_position lidar, lsd_position last, const int* d_pairs, int n_pairs,
                                         double z_occ_max_dis, double max_esti_dist, lsd_match_score* d_out, void* stream) {
    if (!c || !d_map_cache || !d_map_lines || !d_scan_lines || !d_pairs || !d_out || cols <= 0 || rows <= 0 || n_pairs <= 0 ||
        n_points < 0 || (n_points > 0 && !d_pts))
        return LSD_ERR_INVALID;
    if (n_pairs > (1 << 28)) return LSD_ERR_UNSUPPORTED;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_match(d_map_cache, cols, rows, d_map_lines, d_scan_lines, reinterpret_cast<const double*>(d_pts), n_points, lidar.x,
                     lidar.y, last.x, last.y, d_pairs, n_pairs, z_occ_max_dis, max_esti_dist, reinterpret_cast<double*>(d_out), s);
        return LSD_OK;
    });
}

int lsd_scan_to_map_match(lsd_ctx* c, const double* map_cache, int cols, int rows, const lsd_line* map_lines, int n_map,
                          const lsd_line* scan_lines, int n_scan, const lsd_position* pts, int n_points, lsd_position lidar,
                          lsd_position last, const int* pairs, int n_pairs, double z_occ_max_dis, double max_esti_dist,
                          lsd_match_score* out) {
    if (!c || !map_cache || !map_lines || !scan_lines || !pairs || !out || cols <= 0 || rows <= 0 || n_map <= 0 || n_scan <= 0 ||
        n_pairs <= 0 || n_points < 0 || (n_points > 0 && !pts))
        return LSD_ERR_INVALID;
    for (int p = 0; p < n_pairs; p++)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_map || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_scan) return LSD_ERR_INVALID;
    double* d_mc; lsd_line *d_ml, *d_sl; lsd_position* d_pt; int* d_pr; lsd_match_score* d_out;
    auto plan = [&](StagePass& k) {
        k.in(d_mc, map_cache, (size_t)cols * rows); k.in(d_ml, map_lines, n_map); k.in(d_sl, scan_lines, n_scan); k.in(d_pt, pts, n_points);
        k.in(d_pr, pairs, (size_t)n_pairs * 2); k.out(d_out, out, (size_t)n_pairs * 4);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_scan_to_map_match_device(c, d_mc, cols, rows, d_ml, d_sl, d_pt, n_points, lidar, last, d_pr, n_pairs, z_occ_max_dis,
                                                    max_esti_dist, d_out, c->stream);
    });
}

// --- FeatureScan and the scan ingest (k_rdp.hip, k_rdp_long.hip, k_ingest.hip) ---
int lsd_enqueue_feature_scan_batch_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride,
                                          lsd_map_param mp, int region_point_limit, double thre_line, double line_dist_thre_m,
                                          lsd_line* d_lines_out, int* d_n_lines, lsd_position* d_pts_out, int pts_cap, int* d_n_pts,
                                          double* d_lidar_pos, int* d_im_size, void* stream) {
    RdpScans a{};
    a.mapResol = mp.mapResol; a.mapOriX = mp.mapOriX; a.mapOriY = mp.mapOriY;
    return enqueue_feature_scan(c, a, d_scans, d_lens, n_scans, stride, region_point_limit, thre_line, line_dist_thre_m, d_lines_out, d_n_lines,
                                d_pts_out, pts_cap, d_n_pts, d_lidar_pos, d_im_size, stream);
}

int lsd_enqueue_feature_scan_maps_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_scans, int stride,
                                         const lsd_map_ref* maps, int n_maps, const int32_t* d_map_of, int scans_per_seq,
                                         int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line* d_lines_out,
                                         int* d_n_lines, lsd_position* d_pts_out, int pts_cap, int* d_n_pts, double* d_lidar_pos,
                                         int* d_im_size, void* stream) {
    if (!maps) return LSD_ERR_INVALID;
    RdpScans a{};
    a.maps = maps; a.n_maps = n_maps; a.map_of = d_map_of; a.scans_per_seq = scans_per_seq;
    return enqueue_feature_scan(c, a, d_scans, d_lens, n_scans, stride, region_point_limit, thre_line, line_dist_thre_m, d_lines_out, d_n_lines,
                                d_pts_out, pts_cap, d_n_pts, d_lidar_pos, d_im_size, stream);
}

int lsd_enqueue_scan_ingest_device(lsd_ctx* c, const lsd_polar* d_raw, int n_scans, int n_beams, const int* d_take, lsd_polar* d_scans,
                                   int* d_lens, int stride, void* stream) {
    if (!d_raw) return LSD_ERR_INVALID;
    return enqueue_ingest(c, d_raw, nullptr, nullptr, n_scans, n_beams, d_take, d_scans, d_lens, stride, stream);
}

int lsd_enqueue_laserscan_ingest_device(lsd_ctx* c, const float* d_ranges, const float* d_angle_min_inc, int n_scans, int n_beams,
                                        const int* d_take, lsd_polar* d_scans, int* d_lens, int stride, void* stream) {
    if (!d_ranges || !d_angle_min_inc) return LSD_ERR_INVALID;
    return enqueue_ingest(c, nullptr, d_ranges, d_angle_min_inc, n_scans, n_beams, d_take, d_scans, d_lens, stride, stream);
}

int lsd_feature_scan_batch(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_scans, int stride, lsd_map_param mp,
                           int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line* lines_out, int* n_lines,
                           lsd_position* pts_out, int pts_cap, int* n_pts, double* lidar_pos, int* im_size) {
    if (!c || !scans || !lens || n_scans <= 0 || stride <= 0 || !lines_out || !n_lines || !n_pts || !lidar_pos || !im_size || pts_cap < 0 ||
        (pts_cap > 0 && !pts_out))
        return LSD_ERR_INVALID;
    for (int i = 0; i < n_scans; i++) if (lens[i] < 0 || lens[i] > stride) return LSD_ERR_INVALID;
    const size_t ns = (size_t)n_scans;
    lsd_polar* d_sc; int *d_len, *d_nl, *d_np, *d_sz; lsd_line* d_li; lsd_position* d_pt; double* d_lp;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, ns * stride); k.in(d_len, lens, ns); k.out(d_li, lines_out, ns * LSD_RDP_MAX_LINES); k.out(d_pt, pts_out, ns * pts_cap);
        k.out(d_nl, n_lines, ns); k.out(d_np, n_pts, ns); k.out(d_lp, lidar_pos, ns * 2); k.out(d_sz, im_size, ns * 2);
    };
    const int st = stage_round_trip(c, plan, [&] {
        return lsd_enqueue_feature_scan_batch_device(c, d_sc, d_len, n_scans, stride, mp, region_point_limit, thre_line, line_dist_thre_m, d_li, d_nl,
                                                     d_pt, pts_cap, d_np, d_lp, d_sz, c->stream);
    });
    if (st != LSD_OK) return st;
    for (int i = 0; i < n_scans; i++)
        if (n_lines[i] > LSD_RDP_MAX_LINES) return LSD_ERR_CAPACITY;      // more chords than the 360 records per scan hold (the first 360 are valid)
    return LSD_OK;
}

// --- FeatureAssociation: one frame from host arrays ---
void lsd_fa_initial_state(lsd_fa_state* o) {                    // LSD/main_on_windows.cpp:84-93
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->x[0] = -1; o->x[1] = -1;
    const double d[9] = {100, 100, 100, 1, 1, 1, 0.1, 0.1, 0.1};
    for (int i = 0; i < 9; i++) o->P[i * 10] = d[i];
}

int lsd_feature_association(lsd_ctx* c, const double* map_cache, int cols, int rows, const lsd_line* map_lines, int n_map,
                            const lsd_line* scan_lines, int n_scan, const lsd_position* pts, int n_points, lsd_position lidar,
                            lsd_position last, lsd_position sp, const lsd_fa_state* in, lsd_fa_state* out, lsd_fa_report* report) {
    if (!c || !map_cache || cols <= 0 || rows <= 0 || n_map < 0 || n_scan < 0 || n_points < 0 || (n_map > 0 && !map_lines) ||
        (n_scan > 0 && !scan_lines) || (n_points > 0 && !pts) || !in || !out || !report)
        return LSD_ERR_INVALID;
    if ((long long)n_map * n_scan > (1 << 26)) return LSD_ERR_UNSUPPORTED;
    const double sc[8] = {lidar.x, lidar.y, last.x, last.y, last.ang, sp.x, sp.y, sp.ang};
    double *d_mc, *d_sc;                                          // d_sc: lidarPose (2), then lastPose + ScanPose (6)
    lsd_line *d_ml, *d_sl; lsd_position* d_pts; lsd_fa_state *d_in, *d_out; lsd_fa_report* d_rep;
    auto plan = [&](StagePass& k) {
        k.in(d_mc, map_cache, (size_t)cols * rows); k.in(d_ml, map_lines, n_map); k.in(d_sl, scan_lines, n_scan); k.in(d_pts, pts, n_points);
        k.in(d_in, in, 1); k.out(d_out, out, 1); k.out(d_rep, report, 1); k.in(d_sc, sc, 8);
    };
    return stage_round_trip(c, plan, [&] {
        return enqueue_on(c, c->stream, [&](hipStream_t s) -> int {
            FaArgs a{};
            const int r = fa_workspace(c, 1, std::max(1, n_map * n_scan), a);
            if (r != LSD_OK) return r;
            a.map_cache = d_mc; a.cols = cols; a.rows = rows;
            a.map_lines = d_ml; a.n_map = n_map;
            a.scan_lines = d_sl; a.n_lines = nullptr; a.n_scan_given = n_scan; a.line_pitch = std::max(n_scan, 1);
            a.pts = reinterpret_cast<const double*>(d_pts); a.n_pts = nullptr; a.n_pts_given = n_points; a.pts_pitch = std::max(n_points, 1);
            a.lidar_pos = d_sc; a.given = d_sc + 2;
            a.n_frames = nullptr; a.frames_pitch = 1; a.t = 0;
            a.odom = nullptr; a.map_resol = 1;
            a.init = d_in; a.state_in = d_in; a.states = d_out; a.reports = d_rep;
            launch_fa_frame(a, 1, true, s);
            return LSD_OK;
        });
    });
}

int lsd_debug_fa_fuse(lsd_ctx* c, const lsd_match_score* cands, int n, lsd_position last, lsd_position sp, const lsd_fa_state* in,
                      lsd_fa_state* out, lsd_fa_report* report) {
    if (!c || n < 0 || (n > 0 && !cands) || !in || !out || !report) return LSD_ERR_INVALID;
    if (n > (1 << 26)) return LSD_ERR_UNSUPPORTED;
    const double ctl[kFaCtl] = {0, 0, last.x, last.y, last.ang, sp.x, sp.y, sp.ang};
    const int cnt[2] = {0, n};
    lsd_fa_state *d_in, *d_out; lsd_fa_report* d_rep;
    auto plan = [&](StagePass& k) { k.in(d_in, in, 1); k.out(d_out, out, 1); k.out(d_rep, report, 1); };
    return stage_round_trip(c, plan, [&] {
        return enqueue_on(c, c->stream, [&](hipStream_t s) -> int {  // (the candidates go where the matching would have left them: fa_buf)
            FaArgs a{};
            const int r = fa_workspace(c, 1, std::max(1, (n + 3) / 4), a);
            if (r != LSD_OK) return r;
            if (n) HIPCHK(c, hipMemcpyAsync(a.cand, cands, (size_t)n * sizeof(lsd_match_score), hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(a.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(a.n_pairs, &cnt[0], 4, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(a.n_cand, &cnt[1], 4, hipMemcpyHostToDevice, s));
            a.n_frames = nullptr; a.frames_pitch = 1; a.t = 0; a.odom = nullptr;
            a.init = d_in; a.state_in = d_in; a.states = d_out; a.reports = d_rep;
            launch_fa_frame(a, 1, false, s);
            return LSD_OK;
        });
    });
}

// --- the carries: initial value, re-base, correction, relocalisation ---
void lsd_fa_carry_init(lsd_fa_carry* o, const lsd_fa_state* state, lsd_position odom0) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    if (state) o->state = *state;
    else lsd_fa_initial_state(&o->state);
    o->odom = odom0;
}

int lsd_enqueue_fa_carry_rebase_device(lsd_ctx* c, lsd_fa_carry* d_carry, int n_seq, const int32_t* d_key, int32_t key, lsd_map_frame from,
                                       lsd_map_frame to, void* stream) {
    if (!c) return LSD_ERR_INVALID;
    auto bad = [](const lsd_map_frame& f) {
        return !(std::isfinite(f.mapResol) && f.mapResol > 0) || !std::isfinite(f.mapOriX) || !std::isfinite(f.mapOriY);
    };
    if (!d_carry || n_seq <= 0 || bad(from) || bad(to)) return LSD_ERR_INVALID;
    if (from.mapResol == to.mapResol && from.mapOriX == to.mapOriX && from.mapOriY == to.mapOriY) return LSD_OK;   // the same frame: no launch
    return enqueue_on(c, stream, [&](hipStream_t s) {
        const double sc = from.mapResol / to.mapResol;
        const double tx = (from.mapOriX - to.mapOriX) / to.mapResol, ty = (from.mapOriY - to.mapOriY) / to.mapResol;
        launch_fa_rebase(d_carry, n_seq, d_key, key, sc, tx, ty, s);
        return LSD_OK;
    });
}

int lsd_enqueue_fa_carry_correct_device(lsd_ctx* c, lsd_fa_carry* d_carry, int n_seq, int frames_pitch, const void* d_poses, size_t pose_pitch,
                                        const lsd_grid_response_rec* d_resp, const int32_t* d_key, int32_t key, lsd_fa_correct_par par,
                                        lsd_fa_correct_rep* d_rep, void* stream) {
    if (fa_correct_refused(c, d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_resp, d_key, par, d_rep)) return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_fa_correct(d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_resp, d_key, key, par, d_rep, s);
        return LSD_OK;
    });
}

int lsd_fa_carry_correct(lsd_ctx* c, lsd_fa_carry* carries, int n_seq, int frames_pitch, const lsd_position* poses,
                         const lsd_grid_response_rec* resp, lsd_fa_correct_par par, lsd_fa_correct_rep* rep) {
    if (fa_correct_refused(c, carries, n_seq, frames_pitch, poses, sizeof(lsd_position), resp, nullptr, par, rep)) return LSD_ERR_INVALID;
    const size_t ns = (size_t)n_seq, n = ns * (size_t)frames_pitch;
    lsd_fa_carry* d_cy; lsd_position* d_po; lsd_grid_response_rec* d_re; lsd_fa_correct_rep* d_rp;
    auto plan = [&](StagePass& k) { k.both(d_cy, carries, ns); k.in(d_po, poses, n); k.in(d_re, resp, n); k.out(d_rp, rep, ns); };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_fa_carry_correct_device(c, d_cy, n_seq, frames_pitch, d_po, sizeof(lsd_position), d_re, nullptr, 0, par, rep ? d_rp : nullptr,
                                                   c->stream);
    });
}

// Relocalisation (k_falost.hip, k_faseed.hip): the checks of fa_relocate_host.h, then one launch each.
int lsd_enqueue_fa_lost_gather_device(lsd_ctx* c, const lsd_fa_carry* d_carry, int n_seq, int frames_pitch, const void* d_poses, size_t pose_pitch,
                                      const lsd_polar* d_scans, const int* d_lens, int stride, const int32_t* d_key, int32_t key, int max_lost,
                                      lsd_polar* d_scans_out, int* d_lens_out, int32_t* d_pick, int32_t* d_n_lost, void* stream) {
    if (fa_lost_refused(c != nullptr, c ? c->scan_cap : 0, d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_scans, d_lens, stride, d_key, max_lost,
                        d_scans_out, d_lens_out, d_pick, d_n_lost))
        return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_fa_lost_gather(d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_scans, d_lens, stride, d_key, key, max_lost, d_scans_out, d_lens_out,
                              d_pick, d_n_lost, s);
        return LSD_OK;
    });
}

int lsd_fa_lost_gather(lsd_ctx* c, const lsd_fa_carry* carries, int n_seq, int frames_pitch, const lsd_position* poses, const lsd_polar* scans,
                       const int* lens, int stride, int max_lost, lsd_polar* scans_out, int* lens_out, int32_t* pick, int32_t* n_lost) {
    auto there = fa_host_stand_in;                               // (host arrays: the alignment rules are the staging's to keep)
    if (fa_lost_refused(c != nullptr, c ? c->scan_cap : 0, there(carries), n_seq, frames_pitch, there(poses), sizeof(lsd_position), there(scans),
                        there(lens), stride, nullptr, max_lost, there(scans_out), there(lens_out), there(pick), there(n_lost)))
        return LSD_ERR_INVALID;
    const FaLostStage n = fa_lost_stage(n_seq, frames_pitch, stride, max_lost);
    if (fa_lost_bad_len(lens, n.slots, stride) >= 0) return LSD_ERR_INVALID;
    lsd_fa_carry* d_cy; lsd_position* d_po; lsd_polar *d_sc, *d_so; int *d_ln, *d_lo; int32_t *d_pk, *d_nl;
    auto plan = [&](StagePass& k) {                              // (the rows past the gathered ones keep the caller's bytes: scans_out goes both ways)
        k.in(d_cy, carries, n.carries); k.in(d_po, poses, n.slots); k.in(d_sc, scans, n.readings); k.in(d_ln, lens, n.slots);
        k.both(d_so, scans_out, n.readings_out); k.out(d_lo, lens_out, n.rows); k.out(d_pk, pick, n.rows); k.out(d_nl, n_lost, 2);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_fa_lost_gather_device(c, d_cy, n_seq, frames_pitch, d_po, sizeof(lsd_position), d_sc, d_ln, stride, nullptr, 0, max_lost, d_so,
                                                 d_lo, d_pk, d_nl, c->stream);
    });
}

int lsd_enqueue_fa_carry_seed_device(lsd_ctx* c, lsd_fa_carry* d_carry, int n_seq, int frames_pitch, const int32_t* d_pick, int n_pick,
                                     const lsd_grid_locate_rec* d_loc, const lsd_grid_response_rec* d_resp, lsd_fa_seed_par par,
                                     lsd_fa_seed_rep* d_rep, void* stream) {
    if (fa_seed_refused(c != nullptr, d_carry, n_seq, frames_pitch, d_pick, n_pick, d_loc, d_resp, par, d_rep)) return LSD_ERR_INVALID;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_fa_seed(d_carry, n_seq, frames_pitch, d_pick, n_pick, d_loc, d_resp, par, d_rep, s);
        return LSD_OK;
    });
}

int lsd_fa_carry_seed(lsd_ctx* c, lsd_fa_carry* carries, int n_seq, int frames_pitch, const int32_t* pick, int n_pick,
                      const lsd_grid_locate_rec* loc, const lsd_grid_response_rec* resp, lsd_fa_seed_par par, lsd_fa_seed_rep* rep) {
    auto there = fa_host_stand_in;                               // (host arrays: the alignment rules are the staging's to keep)
    if (fa_seed_refused(c != nullptr, there(carries), n_seq, frames_pitch, there(pick), n_pick, there(loc), there(resp), par, there(rep)))
        return LSD_ERR_INVALID;
    const size_t ns = (size_t)n_seq, np = (size_t)n_pick;
    lsd_fa_carry* d_cy; int32_t* d_pk; lsd_grid_locate_rec* d_lc; lsd_grid_response_rec* d_re; lsd_fa_seed_rep* d_rp;
    auto plan = [&](StagePass& k) { k.both(d_cy, carries, ns); k.in(d_pk, pick, np); k.in(d_lc, loc, np); k.in(d_re, resp, np); k.out(d_rp, rep, np); };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_fa_carry_seed_device(c, d_cy, n_seq, frames_pitch, d_pk, n_pick, d_lc, resp ? d_re : nullptr, par, rep ? d_rp : nullptr,
                                                c->stream);
    });
}

// --- the replay loop: each entry's own null checks and its map, then fa_enqueue_loop ---
int lsd_enqueue_localize_device(lsd_ctx* c, const double* d_map_cache, int cols, int rows, const lsd_line* d_map_lines, int n_map,
                                int n_seq, int frames_pitch, const int* n_frames, const lsd_line* d_lines, const int* d_n_lines,
                                const lsd_position* d_pts, int pts_cap, const int* d_n_pts, const double* d_lidar_pos,
                                const lsd_position* d_odom, double map_resol, const lsd_fa_state* d_init, lsd_fa_state* d_states,
                                lsd_fa_report* d_reports, void* stream) {
    if (!d_init) return LSD_ERR_INVALID;
    const FaLoopMap map = {.d_map_cache = d_map_cache, .cols = cols, .rows = rows, .d_map_lines = d_map_lines, .n_map = n_map, .map_resol = map_resol};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, d_init,
                                             nullptr, d_states, d_reports), stream);
}

int lsd_enqueue_localize_resume_device(lsd_ctx* c, const double* d_map_cache, int cols, int rows, const lsd_line* d_map_lines, int n_map,
                                       int n_seq, int frames_pitch, const int* n_frames, const lsd_line* d_lines, const int* d_n_lines,
                                       const lsd_position* d_pts, int pts_cap, const int* d_n_pts, const double* d_lidar_pos,
                                       const lsd_position* d_odom, double map_resol, lsd_fa_carry* d_carry, lsd_fa_state* d_states,
                                       lsd_fa_report* d_reports, void* stream) {
    if (!d_carry) return LSD_ERR_INVALID;
    const FaLoopMap map = {.d_map_cache = d_map_cache, .cols = cols, .rows = rows, .d_map_lines = d_map_lines, .n_map = n_map, .map_resol = map_resol};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, nullptr,
                                             d_carry, d_states, d_reports), stream);
}

int lsd_enqueue_localize_live_map_device(lsd_ctx* c, const double* d_map_cache, int cols, int rows, const lsd_line* d_map_lines,
                                         int map_lines_cap, const int32_t* d_n_map, int n_seq, int frames_pitch, const int* n_frames,
                                         const lsd_line* d_lines, const int* d_n_lines, const lsd_position* d_pts, int pts_cap,
                                         const int* d_n_pts, const double* d_lidar_pos, const lsd_position* d_odom, double map_resol,
                                         const lsd_fa_state* d_init, lsd_fa_state* d_states, lsd_fa_report* d_reports, void* stream) {
    if (!d_init || !d_n_map || map_lines_cap <= 0) return LSD_ERR_INVALID;
    const FaLoopMap map = {.d_map_cache = d_map_cache, .cols = cols, .rows = rows, .d_map_lines = d_map_lines, .n_map = map_lines_cap,
                           .d_n_map = d_n_map, .map_resol = map_resol};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, d_init,
                                             nullptr, d_states, d_reports), stream);
}

int lsd_enqueue_localize_resume_live_map_device(lsd_ctx* c, const double* d_map_cache, int cols, int rows, const lsd_line* d_map_lines,
                                                int map_lines_cap, const int32_t* d_n_map, int n_seq, int frames_pitch, const int* n_frames,
                                                const lsd_line* d_lines, const int* d_n_lines, const lsd_position* d_pts, int pts_cap,
                                                const int* d_n_pts, const double* d_lidar_pos, const lsd_position* d_odom, double map_resol,
                                                lsd_fa_carry* d_carry, lsd_fa_state* d_states, lsd_fa_report* d_reports, void* stream) {
    if (!d_carry || !d_n_map || map_lines_cap <= 0) return LSD_ERR_INVALID;
    const FaLoopMap map = {.d_map_cache = d_map_cache, .cols = cols, .rows = rows, .d_map_lines = d_map_lines, .n_map = map_lines_cap,
                           .d_n_map = d_n_map, .map_resol = map_resol};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, nullptr,
                                             d_carry, d_states, d_reports), stream);
}

int lsd_enqueue_localize_maps_device(lsd_ctx* c, const lsd_map_ref* maps, int n_maps, const int32_t* d_map_of, int n_seq, int frames_pitch,
                                     const int* n_frames, const lsd_line* d_lines, const int* d_n_lines, const lsd_position* d_pts,
                                     int pts_cap, const int* d_n_pts, const double* d_lidar_pos, const lsd_position* d_odom,
                                     const lsd_fa_state* d_init, lsd_fa_state* d_states, lsd_fa_report* d_reports, void* stream) {
    if (!d_init) return LSD_ERR_INVALID;
    const FaLoopMap map = {.maps = maps, .n_maps = n_maps, .d_map_of = d_map_of};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, d_init,
                                             nullptr, d_states, d_reports), stream);
}

int lsd_enqueue_localize_resume_maps_device(lsd_ctx* c, const lsd_map_ref* maps, int n_maps, const int32_t* d_map_of, int n_seq,
                                            int frames_pitch, const int* n_frames, const lsd_line* d_lines, const int* d_n_lines,
                                            const lsd_position* d_pts, int pts_cap, const int* d_n_pts, const double* d_lidar_pos,
                                            const lsd_position* d_odom, lsd_fa_carry* d_carry, lsd_fa_state* d_states,
                                            lsd_fa_report* d_reports, void* stream) {
    if (!d_carry) return LSD_ERR_INVALID;
    const FaLoopMap map = {.maps = maps, .n_maps = n_maps, .d_map_of = d_map_of};
    return fa_enqueue_loop(c, map, fa_frames(n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, nullptr,
                                             d_carry, d_states, d_reports), stream);
}

int lsd_localize(lsd_ctx* c, const double* map_cache, int cols, int rows, const lsd_line* map_lines, int n_map, const lsd_polar* scans,
                 const int* lens, int n_frames, int stride, const lsd_position* odom, lsd_map_param mp, const lsd_fa_state* init,
                 lsd_fa_state* states, lsd_fa_report* reports) {
    if (!c || !map_cache || cols <= 0 || rows <= 0 || n_map < 0 || (n_map > 0 && !map_lines) || !scans || !lens || n_frames <= 0 ||
        stride <= 0 || !odom || !states || !reports || !(mp.mapResol > 0))
        return LSD_ERR_INVALID;
    for (int i = 0; i < n_frames; i++) if (lens[i] < 0 || lens[i] > stride) return LSD_ERR_INVALID;
    if (stride > c->scan_cap) return LSD_ERR_UNSUPPORTED;
    const int pts_cap = 8192;
    const size_t nf = (size_t)n_frames;
    lsd_fa_state h_init;
    if (init) h_init = *init;
    else lsd_fa_initial_state(&h_init);
    std::vector<int> nl(nf), np(nf);
    double *d_mc, *d_lp; lsd_line *d_ml, *d_lines; lsd_polar* d_scans; int *d_lens, *d_nl, *d_np, *d_sz; lsd_position *d_odom, *d_pts;
    lsd_fa_state *d_init, *d_states; lsd_fa_report* d_reports;
    auto plan = [&](StagePass& k) {
        k.in(d_mc, map_cache, (size_t)cols * rows); k.in(d_ml, map_lines, n_map); k.in(d_scans, scans, nf * stride); k.in(d_lens, lens, nf);
        k.in(d_odom, odom, nf + 1); k.in(d_init, &h_init, 1); k.scratch(d_lines, nf * LSD_RDP_MAX_LINES); k.out(d_nl, nl.data(), nf);
        k.scratch(d_pts, nf * pts_cap); k.out(d_np, np.data(), nf); k.scratch(d_lp, nf * 2); k.scratch(d_sz, nf * 2); k.out(d_states, states, nf);
        k.out(d_reports, reports, nf);
    };
    const int st = stage_round_trip(c, plan, [&] {
        const int r = lsd_enqueue_feature_scan_batch_device(c, d_scans, d_lens, n_frames, stride, mp, 3, 0.08, 0.5, d_lines, d_nl, d_pts, pts_cap, d_np,
                                                            d_lp, d_sz, c->stream);   // rdp defaults, baseFunc.h:70-72
        if (r != LSD_OK) return r;
        return lsd_enqueue_localize_device(c, d_mc, cols, rows, d_ml, n_map, 1, n_frames, &n_frames, d_lines, d_nl, d_pts, pts_cap, d_np, d_lp, d_odom,
                                           mp.mapResol, d_init, d_states, d_reports, c->stream);
    });
    if (st != LSD_OK) return st;
    for (size_t i = 0; i < nf; i++)
        if (nl[i] > LSD_RDP_MAX_LINES || np[i] > pts_cap) return LSD_ERR_CAPACITY;
    return LSD_OK;
}

}  // extern "C"
