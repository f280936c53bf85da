// lsd_internal.h -- shared between the host side (lsd_ctx.hip, lsd_loc.hip, lsd_grid.hip, lsd_pg.hip, lsd_dist.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lsd_hip.h"

namespace lsdhip {

constexpr double kPi = 3.14159265358979323846;  // == 4.0*atan(1.0), myLSD.cpp:9
constexpr int kCentreCount = 32768;             // scaled coordinates are below 32766 (make_geom)
constexpr int kMaxTapRadius = 40;               // hSize = 2*h+1 <= 81 taps per phase kernel
constexpr int kLgTable = 16384;                 // host-tabulated log-gamma entries every context starts with; it grows to w*h + 2 (the largest
constexpr int kLgTableMax = 1 << 23;            //    pixel count a rectangle can have, + 1), up to this many
constexpr int kStatWords = 48;                  // counters per image of the region stage (lsd_debug_fetch LSD_DBG_STATS)
constexpr int kStatTiesWord = 39;               // ... and this one its decisions within the libm's noise (region/stats.h: ST_TIES; lsd_last_sensitivity)
constexpr int kStatGrowAnyWord = 45;            // ... bits 8.. of this one count the calls of grow_any() (region/grow.h; region/stats.h: ST_GROWANY), bits 3..0: the XCC the image ran on
constexpr int kStatTotalWord = 8;               // ... of which this one holds the shader clocks the stage spent on the image (region/stats.h: ST_TOTAL)
constexpr int kPTable = 16;                     // host-tabulated log(p), log10(p), log(1-p) for p = aliPro/2^k
// Help across workgroups in the region stage (k_region.hip): a control block of 32-bit words per launch, cleared before it.
//   per image (kXStride words): [0] accept epoch [1] commit cursor [2] image finished [3] helper wavefronts attached
//   [4] seeds waiting for a full evaluation; [R, 2R) requests (seed + 1, bit 31: taken by a helper); [2R, 3R) flags of the
//   answers (seed + 1); [3R, 11R) the answers, 8 words each: result state, result slot, accept epoch of the snapshot, box (2),
//   list sizes (R = kXReq).  After the n image records (kXHdr words): [0] workgroups started [1] images finished [2] length
//   of the list of images that ask for help [3] early helper wavefronts [4] s_memrealtime of the launch's start | 1; the list (image + 1) follows.
constexpr int kXStride = 768, kXReq = 64, kXHdr = 16;

// Geometry + thresholds of one (cols, rows, params) configuration; computed on the host with the
// host libm so that they are the very numbers the reference computes (myLSD.cpp:132-133,148-149,207-209).
struct Geom {
    int W, H;            // original size
    int w, h;            // scaled size
    int npx;             // w*h
    int gp;              // row pitch (doubles) of the Gaussian image: w rounded up to 16, so that every row starts on a 128-byte line
    double sca;
    int tapR;            // Gaussian tap radius h (myLSD.cpp:393)
    int pseBin;
    double degThre;      // angThre/180*pi
    double gradThre;     // 2/sin(degThre)
    double logNT;        // 5*(log10(h)+log10(w))/2
    double regThre;      // -logNT/log10(angThre/180)
    double aliPro;       // angThre/180
    double denThre;
};

// The packed pixel word pw[q] of the scaled image (written by K2, read by the region stage):
//   bits 31..2  the level-line angle degMap[q] as fp32 with the two lowest mantissa bits cleared (|error| < 1e-6 rad)
//   bits  1..0  usedMap code: 0 free, 1 banned by the gradient threshold (myLSD.cpp:165-166), 2 marked by a rejected
//               region (usedMap == 2: growable, not seedable), 3 banned by an accepted line (usedMap == 1; the line's
//               epoch is in epochmap[q], written before the code).  usedMap value = code == 3 ? 1 : code.
constexpr uint32_t kPwFree = 0u, kPwStatic = 1u, kPwRejected = 2u, kPwLine = 3u;
__host__ __device__ inline uint32_t pw_used(uint32_t w) { return (w & 3u) == 3u ? 1u : (w & 3u); }

// Per-batch device buffers (image i lives at base + i*stride of each array).
struct Buffers {
    const uint8_t* in;     // n x H x W (pitch W)
    uint8_t* in_rw;        // same pointer when write-back of the remap is requested, else null
    double* gauss;         // n x h x gp (row pitch gp: see Geom); null on the fused front end's path
    double* mag;           // n x npx
    double* deg;           // n x npx
    double2* sc;           // n x npx : (sin, cos)(deg), written where usedMap == 0 after the gradient pass
    uint32_t* pw;          // n x npx : packed pixel word (see above)
    uint32_t* epochmap;    // n x npx : accept epoch of pixels with code 3; for growable pixels the label of their certified set, tagged with the run number (region/config.h: label_make; cleared with the stamps when the run numbers wrap)
    uint32_t* sets;        // n x 256 : sizes of the certified sets of the launch by label, 0 = none / ended (cleared by the region stage itself)
    uint32_t* tepoch;      // n x ceil(w/8) x ceil(h/8) : per tile, epoch + 1 of the latest accepted line with a pixel in it (cleared per run)
    unsigned long long* maxbits;  // n : bit pattern of max gradient (non-negative double)
    int32_t* nb;           // n : sorted-list length
    int32_t* ties;         // n : decisions of the gradient pass within the libm's noise (lsd_last_sensitivity; the region stage counts its own in the counter records)
    uint32_t* ord;         // n x npx : sorted seed list (y*w+x)
    uint32_t* stamps;      // n x NW x tm_stride : per wave, the member masks of the tiles its cache has evicted (4 words per 8x8 tile: grow id, -, 64 bits)
    int tm_stride;         // words per wave of the above: 4 x tiles of the scaled image
    uint32_t* spill;       // n x NW x npx : region list beyond the LDS part
    uint32_t* gcopy;       // n x NW x npx : grow-order copy used when RegionRadiusReducer reorders the list
    float4* wmeta;         // n x NW x mcap : per list entry (unit sum vector, sin of the smallest slack) of its last neighbourhood test
    int mcap;
    int* rnum;             // n x RW x 2 : sizes/outcome of published records (seed trace only)
    uint32_t* order;       // n : image indices, heaviest (largest nb) first: the region stage's workgroup -> image map
    uint32_t* seedidx;     // n x npx : sorted-list indices of the potential seeds (usedMap == 0 after the gradient pass)
    uint32_t* seedpos;     // n x npx : their pixels (y*w+x), same order
    uint32_t* slist;       // n x NW x NS x gcap : lists of the speculative results in flight (examined pixels, pixels to mark)
    int gcap;
    uint32_t id_budget;    // curMap stamp ids per wave and run (region/grow.h: grow())
    int tun_soft, tun_claim, tun_feed, tun_big;   // schedule of the region stage (k_region.hip; lsd_ctx.hip has the defaults)
    uint32_t* xq;          // n x kXStride + kXHdr + n : control block of the help across workgroups (see above), null: no help
    int tun_help;          // helper wavefronts an image may have attached
    int* pcount;           // persistent workgroups of the 8-wave region stage (k_region.hip: k_region; lsd_ctx.hip: tun_groups): the launch's image counter (zeroed before the launch), else null
    int nimg;              // ... and the number of images its workgroups share out
    int npool;             // workgroups at the end of the region stage's launch that own no image and help from the start (workspace slots n .. n + npool - 1)
    int tun_early;         // workgroups that may help while others still wait for a CU
    int tun_wb;            // an image asks for help while its waves idle less than this share of the time (percent)
    int tun_gate;          // ... and once it has been running for this long (1024-clock units)
    int tun_share;         // ... and for at least this share (percent) of the time since the launch began
    int tun_up, tun_down;  // steps of the adaptive look-ahead (seeds): up when a wave finds nothing to do, down on a redo / discard
    int tun_requeue;       // results invalidated by a line are queued for another evaluation when the line is accepted (1) or found at the cursor (0)
    int tun_xpoll;         // shader clocks between two looks of a wave at the help protocol
    int tun_linger;        // looks (~27 us each) a helper wavefront takes for an image that asks before it gives its CU back
    int tun_stop;          // experiments: the seed loop ends after this many potential seeds (0: all)
    double* pend;          // n x NW x NS x 24 : finished results that mark usedMap, waiting for their turn to commit
    double* recs;          // n x max_lines x 12 (structRec before rescale)
    double* recs_scaled;   // n x max_lines x 4 (x1 y1 x2 y2 after the 1/sca rescale)
    int32_t* counts;       // n
    lsd_line* lines;       // n x max_lines
    uint8_t* line_im;      // n x H x W or null
    int max_lines;
    // tables
    const double* taps;    // 3 x (2*tapR+1)
    const int* centres;    // kCentreCount: (int)floor(x / sca + 0.5) for every scaled coordinate x (K1's window centres, myLSD.cpp:428 / :460)
    const double* lgamma;  // lg_count entries: LogGammaCalculator(i) from the host libm
    int lg_count;
    const double* ptab;    // kPTable x 3 : log(p), log10(p), log(1-p)
    // debug
    void* seeds;           // n x npx trace records or null
    int32_t* nseed;        // n
    long long* stats;      // n x kStatWords
    int fuse_lines;        // the region stage's workgroup writes the lines of an image it has finished (lines_dev.h): no k_lines behind it (lsd_ctx.hip says when)
};

struct SeedRec {  // mirrors oracle's orc_seed
    int order_idx, x, y, num, outcome, final_num;
    double logNFA;
};

// launchers (each enqueues on `s`)
hipError_t prepare_gauss(const Geom& g);   // raises K1's dynamic-LDS limit where its window needs it; called before a call enqueues anything
void launch_gauss(const Geom& g, const Buffers& b, int n, uint8_t* clr, bool remapped, hipStream_t s);   // clr: lineIm to be cleared on the way, or null; remapped: b.in holds remapped values already
// the fused front end (k_front.hip): K1 + K2 in one kernel for the reference's 17 taps, without the Gaussian image (b.gauss is not used)
bool front_fits(const Geom& g, size_t max_lds);   // 17 taps and its LDS (k_front_lds.h) within the device's and the default launch limit
void launch_front(const Geom& g, const Buffers& b, int n, uint8_t* clr, hipStream_t s);
void launch_remap_writeback(const Geom& g, const Buffers& b, int n, hipStream_t s);
void launch_gradient(const Geom& g, const Buffers& b, int n, hipStream_t s);
void launch_sort(const Geom& g, const Buffers& b, int n, hipStream_t s);
void launch_ordv(const double* mag, const unsigned long long* maxbits, const uint32_t* ord, uint16_t* out, int count, int pseBin, hipStream_t s);   // debug fetch of the bin values
void launch_order(const Buffers& b, int n, int npx, const long long* hist, hipStream_t s);   // hist: the last launch's counter records (cost history) or null
// the region stage with 4 resp. 8 wavefronts per image (k_region.hip is compiled twice)
void launch_region_w4(const Geom& g, const Buffers& b, int n, uint32_t id_base, hipStream_t s);
void launch_region_w8(const Geom& g, const Buffers& b, int n, uint32_t id_base, hipStream_t s);
int region_slots();    // result slots per wavefront (slist and pend are sized x this)
int region_waves();    // wavefronts per image of the wider variant: what the workspace is sized for
int region_ring();     // commit-ring records per image (rnum is sized x this x 2)
void launch_calib(double* buf, size_t n, hipStream_t s);
void launch_match(const double* map_cache, int cols, int rows, const lsd_line* map_lines, const lsd_line* scan_lines,
                  const double* pts, int n_points, double lidx, double lidy, double lastx, double lasty, const int* pairs,
                  int n_pairs, double zmax, double max_esti_dist, double* out, hipStream_t s);
void launch_occ_to_map(const uint8_t* in, uint8_t* out, size_t n, hipStream_t s);
void launch_mapcache_spread(const uint8_t* maps, double* out, unsigned long long* claim, uint32_t* fr_a, uint32_t* fr_b, int* ctl,
                            int* cnt, int n, int G, int W, int H, double res, double zmax, int cell_radius, hipStream_t s);
void launch_mapcache(const uint8_t* maps, double* out, unsigned long long* claim, uint32_t* fr_a, uint32_t* fr_b, int n,
                     int W, int H, double res, double zmax, int cell_radius, hipStream_t s);
void launch_lines(const Geom& g, const Buffers& b, int n, hipStream_t s);
// K5 on one image's caller-given rectangles (lsd_debug_lines): n records, a capacity of n, an image of W x H cells
void launch_lines_of(const double* recs_scaled, const int32_t* count, lsd_line* lines, uint8_t* line_im, int n, int W, int H, hipStream_t s);
void launch_clear(uint8_t* p, size_t bytes, int num_cus, hipStream_t s);   // lineIm = zeros (k_lines.hip)
void launch_compact_lines(const lsd_line* lines, const int32_t* counts, int max_lines, int n, lsd_line* flat, int32_t* offsets, hipStream_t s);
// FeatureScan (k_rdp.hip for strides up to kRdpShortMaxLen of k_rdp_lds.h, k_rdp_long.hip above: launch_rdp chooses).  What a launch
// reads: n scans at `stride` readings each with the rdp parameters and the map's mapResol / mapOriX / mapOriY -- the three scalars
// where maps is null, else those of scan i read from maps[map_of[i / scans_per_seq]] (a device table of n_maps records; a scan whose
// id is outside 0..n_maps-1 gets counts 0 and nothing else).  And what it writes, per scan: LSD_RDP_MAX_LINES records, pts_cap pixels,
// the two counts, lidar_pos and im_size (two values each)
struct RdpScans { const double* scans; const int* lens; int n, stride; int region_point_limit; double thre_line, line_dist_thre_m;
                  double mapResol, mapOriX, mapOriY; const lsd_map_ref* maps; int n_maps; const int32_t* map_of; int scans_per_seq; };
struct RdpOut { lsd_line* lines; int* n_lines; double* pts; int pts_cap; int* n_pts; double* lidar_pos; int* im_size; };
void launch_rdp(const RdpScans& a, const RdpOut& o, hipStream_t s);
// the long kernels' dynamic LDS is rdp_long_lds(stride) bytes (k_rdp_lds.h), for which prepare_rdp_long raises their limit where it is
// above 64 KiB
hipError_t prepare_rdp_long(size_t bytes);
// the drivers' scan read loop (k_ingest.hip): raw (pairs) or ranges + min_inc (LaserScan) -> scans / lens as launch_rdp reads them
void launch_ingest(const lsd_polar* raw, const float* ranges, const float* min_inc, int n, int n_beams, const int* take, lsd_polar* scans,
                   int* lens, int stride, hipStream_t s);
// The grid stack (host side: lsd_grid.hip).  The scans of a frame as its four scan-taking launchers receive them: n_scans scans as
// launch_rdp reads them, each at the pose in the first three doubles of the record at poses + i * pose_pitch, in a cols x rows grid of
// resol metres a cell, beams cut at range_max
struct GridScans { const lsd_polar* scans; const int* lens; int n_scans, stride; const void* poses; size_t pose_pitch;
                   int cols, rows; double resol, range_max; };
// mapping with known poses (k_gridmap.hip): the scans counted into the two planes of the grid; and a pair of planes published as an int8 grid
void launch_grid_integrate(const GridScans& g, uint32_t* pass, uint32_t* hit, hipStream_t s);
void launch_grid_publish(const uint32_t* pass, const uint32_t* hit, size_t n_cells, uint32_t min_pass, uint32_t occ_num, uint32_t occ_den,
                         int8_t* grid, hipStream_t s);
// correlative scan-to-grid matching (k_gridmatch.hip): the lookup plane of a pair of counter planes; and the scans matched on it around
// their poses, through `slots` (grid_match_slot_bytes(n_scans, na) bytes of workspace) into n_scans records
void launch_grid_likelihood(const uint32_t* pass, const uint32_t* hit, int cols, int rows, uint32_t min_pass, uint32_t occ_num, uint32_t occ_den,
                            const lsd_grid_smear& smear, uint8_t* corr, hipStream_t s);
size_t grid_match_slot_bytes(int n_scans, int na);
void launch_grid_match(const GridScans& g, const uint8_t* corr, const lsd_grid_search& se, void* slots, lsd_grid_match_rec* out, hipStream_t s);
void launch_grid_match_pick(int n_scans, const void* poses, size_t pose_pitch, const lsd_grid_search& se, const void* slots, lsd_grid_match_rec* out,
                            hipStream_t s);
// the same match as a coarse-to-fine search (k_gridmatch_mr.hip): the plane of block maxima ((rows + block - 1) x (cols + block - 1)
// bytes), and the match through four regions of workspace -- U, the coarse slots, the counts, the slots of launch_grid_match_pick --
// whose sizes grid_match_mr_ws gives; stats may be null
void launch_grid_coarse(const uint8_t* corr, int cols, int rows, int block, uint8_t* coarse, hipStream_t s);
void grid_match_mr_ws(int n_scans, const lsd_grid_search& se, int block, size_t bytes[4]);
void launch_grid_match_mr(const GridScans& g, const uint8_t* corr, const uint8_t* coarse, int block, const lsd_grid_search& se, void* const ws[4],
                          lsd_grid_match_rec* out, lsd_grid_match_mr_stats* stats, hipStream_t s);
// the response around a match (k_gridresponse.hip): the records of either search -> the volume of R (grid_response_volume_bytes bytes,
// the caller's or workspace) -> n_scans response records
size_t grid_response_volume_bytes(int n_scans, const lsd_grid_response_par& rp);
void launch_grid_response(const GridScans& g, const lsd_grid_match_rec* records, const uint8_t* corr, double ang_step, const lsd_grid_response_par& rp,
                          uint32_t* volume, lsd_grid_response_rec* out, hipStream_t s);
// ray casting on the grid (k_gridray.hip): per beam the expected range and its class against the int8 grid, per scan the summary (and the
// gate), and with scans_out (may be null, may be g.scans) the screened readings; two launches, no workspace
void launch_grid_raycast(const GridScans& g, const int8_t* grid, const lsd_grid_ray_par& par, lsd_grid_ray* out, lsd_grid_ray_sum* sum,
                         lsd_polar* scans_out, hipStream_t s);
// global scan-to-grid localisation (k_gridlocate.hip): the pyramid of block maxima of a lookup plane (levels 0..levels one behind the other,
// level h at grid_pyramid_offset), and the scans located in a box of cells and a fan of headings through kGridLocateRegions regions of
// workspace -- the offsets, nb, L_a, the dense U_H, two node lists, the counters, the slots -- whose sizes grid_locate_ws gives; stats may
// be null
constexpr int kGridLocateRegions = 8;
size_t grid_pyramid_offset(int cols, int rows, int h);
void launch_grid_pyramid(const uint8_t* corr, int cols, int rows, int levels, uint8_t* pyramid, hipStream_t s);
size_t grid_locate_top_nodes(const lsd_grid_locate_par& par);
void grid_locate_ws(int n_scans, int stride, const lsd_grid_locate_par& par, size_t bytes[kGridLocateRegions]);
void launch_grid_locate(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                        const uint8_t* pyramid, const lsd_grid_locate_par& par, void* const ws[kGridLocateRegions], lsd_grid_locate_rec* out,
                        lsd_grid_locate_stats* stats, hipStream_t s);
// the tight search (k_gridlocate_tight.hip): the same regions and two more -- kLocTight words per scan, a 64-bit key per scan and heading
constexpr int kGridLocateTightRegions = kGridLocateRegions + 2;
void grid_locate_tight_ws(int n_scans, int stride, const lsd_grid_locate_par& par, size_t bytes[kGridLocateTightRegions]);
void launch_grid_locate_tight(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                              const uint8_t* pyramid, const lsd_grid_locate_par& par, uint32_t tight, void* const ws[kGridLocateTightRegions],
                              lsd_grid_locate_rec* out, lsd_grid_locate_tight_stats* stats, hipStream_t s);
void launch_pack_lines(const lsd_line* lines, const int32_t* counts, int n_local, int max_lines, int per, int cap_rows, int32_t* cpad,
                       int32_t* offs, lsd_line* slab, hipStream_t s);
// Device FeatureAssociation (k_fa.hip): one frame index of n_seq sequences.  Frame t of sequence s lives in slot s * frames_pitch + t
// of the per-frame arrays; the workspace arrays are per sequence (pairs: pair_cap x 2 ints, cand: 4 pair_cap x 4 doubles, scratch:
// 8 pair_cap ints, ctl: kFaCtl doubles {lidarPose x, y, lastPose x, y, ang, ScanPose x, y, ang}, aux: kFaAux doubles {sum of
// angRotate, its length, is_offset, frames consumed}).
// carry (not null): the resumable loop (lsd_enqueue_localize_resume_device).  The previous state, the bookkeeping and Odom[cnt_frame - 1]
// of frame 0 come from carry[s]; odom then holds frames_pitch NEW rows per sequence (frame t: Odom[cnt_frame] = row t), and the fuse
// kernel of a sequence's last frame writes the loop's variables back to carry[s].
// maps (not null): the fleet entries (lsd_enqueue_localize*_maps_device).  Sequence s runs against maps[map_of[s]], a device table of
// n_maps records, in place of the single-map fields; an id outside 0..n_maps-1 makes the sequence sit the call out (fa_map, k_fa.hip).
constexpr int kFaCtl = 8, kFaAux = 4, kFaLdsMax = 1024;
struct FaArgs {
    const double* map_cache; int cols, rows;
    const lsd_line* map_lines; int n_map; const int32_t* d_n_map;                       // d_n_map (not null): the count lives on the device, n_map is its capacity
    const lsd_line* scan_lines; const int* n_lines; int n_scan_given; int line_pitch;   // n_lines null: n_scan_given lines
    const double* pts; const int* n_pts; int n_pts_given; int pts_pitch;                // n_pts null: n_pts_given points
    const double* lidar_pos;                                                            // 2 per slot
    const int* n_frames; int frames_pitch, t;                                           // n_frames null: every sequence has frame t
    const lsd_position* odom;                                                           // (frames_pitch + 1) rows per sequence, or null
    lsd_fa_carry* carry;                                                                // null, or n_seq carries (odom: frames_pitch rows)
    const double* given;                                                                // null, or 6 per sequence: lastPose, ScanPose
    double map_resol;
    const lsd_map_ref* maps; const int32_t* map_of; int n_maps;                         // maps null: the single map above
    const lsd_fa_state* init; const lsd_fa_state* state_in;                             // state_in (not null): the fuse kernel's input
    lsd_fa_state* states; lsd_fa_report* reports;
    int* pairs; int* n_pairs; int* n_cand; int pair_cap;
    double* cand; int* scratch; double* ctl; double* aux;
    int lds_bound;
};
void launch_fa_frame(const FaArgs& a, int n_seq, bool prepare, hipStream_t s);   // prepare = false: the fuse kernel alone (ctl, cand, counts given)
// carries from one map frame to another, in place (k_fa.hip: k_fa_rebase): x[0..1] scaled and shifted, the rates and P scaled
void launch_fa_rebase(lsd_fa_carry* carry, int n_seq, const int32_t* key_of, int32_t key, double sc, double tx, double ty, hipStream_t s);
// the grid match response fused into the carries, in place (k_facorrect.hip: k_fa_correct): one launch, no workspace
void launch_fa_correct(lsd_fa_carry* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch, const lsd_grid_response_rec* resp,
                       const int32_t* key_of, int32_t key, lsd_fa_correct_par par, lsd_fa_correct_rep* rep, hipStream_t s);
// relocalisation (k_falost.hip: k_fa_lost_gather; k_faseed.hip: k_fa_seed): one launch each, no workspace
void launch_fa_lost_gather(const lsd_fa_carry* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch, const lsd_polar* scans,
                           const int* lens, int stride, const int32_t* key_of, int32_t key, int max_lost, lsd_polar* scans_out, int* lens_out,
                           int32_t* pick, int32_t* n_lost, hipStream_t s);
void launch_fa_seed(lsd_fa_carry* carry, int n_seq, int frames_pitch, const int32_t* pick, int n_pick, const lsd_grid_locate_rec* loc,
                    const lsd_grid_response_rec* resp, lsd_fa_seed_par par, lsd_fa_seed_rep* rep, hipStream_t s);
// the pose graph (host side: lsd_pg.hip).  What near, recognize and loop_select leave for a closure chain (posegraph_dev.h: pg_hand_over):
// the near record, the selection of nodes_cap poses, the query's row of store_stride readings, its length and the pose the search starts from
struct PgHandOver { lsd_pg_near_rec* rec; lsd_position* sel; lsd_polar* q_scan; int* q_len; lsd_position* q_pose; };
// Building it (k_pgbuild.hip): one launch each, no workspace
void launch_pg_append(const lsd_polar* scans, const int* lens, int n_cand, int stride, const void* poses, size_t pose_pitch, lsd_pg_head* head,
                      lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* track, int32_t track_id, lsd_polar* store,
                      int* store_lens, int store_stride, lsd_pg_append_par par, lsd_pg_append_rep* rep, hipStream_t s);
void launch_pg_near(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track, const lsd_polar* store,
                    const int* store_lens, int store_stride, int gap, double radius, int window, PgHandOver out, hipStream_t s);
void launch_pg_closure(lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, const lsd_pg_near_rec* near_rec,
                       const lsd_grid_response_rec* resp, lsd_pg_closure_par par, lsd_pg_closure_rep* rep, hipStream_t s);
// its relaxation (k_posegraph.hip): one workgroup per graph; pg_ws_bytes: the workspace of one graph
size_t pg_ws_bytes(int nodes_cap, int edges_cap);
void launch_pg_relax(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                     lsd_pg_relax_par par, void* ws, lsd_pg_relax_rep* rep, hipStream_t s);
// the same body with a robust kernel on the edges (rob_rep may be null), and the rejection of closures by their chi2 (k_pgprune.hip)
void launch_pg_relax_robust(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                            lsd_pg_relax_par par, lsd_pg_robust_par rob, void* ws, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep, hipStream_t s);
void launch_pg_prune(int n_graphs, const lsd_pg_head* heads, lsd_pg_edge* edges, int edges_cap, lsd_pg_prune_par par, lsd_pg_prune_rep* rep,
                     hipStream_t s);
// the robust body with the block-tridiagonal preconditioner (k_pgchain.hip; rob_rep and pc_rep may be null); pg_ws_pc_bytes: the workspace
// of one graph for a kind of preconditioner
size_t pg_ws_pc_bytes(int nodes_cap, int edges_cap, int kind);
void launch_pg_relax_chain(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                           lsd_pg_relax_par par, lsd_pg_robust_par rob, void* ws, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep,
                           lsd_pg_precond_rep* pc_rep, hipStream_t s);
// marginal covariances and the gate on new closures (k_pgmarg.hip): prepare (one workgroup) and solve (min(n_q, slots) workgroups) on one
// stream, prior may be null; pg_marg_ws_bytes: the shared part (pg_ws_pc_bytes) and `slots` slices of pg_marg_slice_bytes; the vet is one
// workgroup (reps may be null)
size_t pg_marg_slice_bytes(int nodes_cap, int kind);
size_t pg_marg_ws_bytes(int nodes_cap, int edges_cap, int kind, int slots);
void launch_pg_marginals(const lsd_pg_head* head, const lsd_pg_head* prior, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_edge* edges,
                         int edges_cap, const lsd_pg_marg_query* queries, int n_q, lsd_pg_marg_par par, void* ws, lsd_pg_marg_rec* recs,
                         lsd_pg_marg_rep* rep, hipStream_t s);
void launch_pg_vet(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                   const lsd_pg_marg_query* queries, const lsd_pg_marg_rec* recs, int n_q, double gate, lsd_pg_vet_rep* reps, hipStream_t s);
// place recognition (k_pgplace.hip): the descriptors of the rows that have none; and score + pick (out.rec == nullptr: the records and
// the report only -- nodes, store, store_lens and the rest of out are not read or written then)
void launch_pg_describe(const lsd_pg_head* head, int nodes_cap, const lsd_polar* store, const int* store_lens, int store_stride, double range_max,
                        lsd_pg_desc* desc, hipStream_t s);
void launch_pg_recognize(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track, const lsd_polar* store,
                         const int* store_lens, int store_stride, const lsd_pg_desc* desc, lsd_pg_place_par par, uint32_t* work,
                         lsd_pg_place_rec* recs, lsd_pg_place_rep* rep, PgHandOver out, hipStream_t s);
// every loop of a track (k_pgloops.hip): a range of queries in one launch (an error of the runtime before anything is queued is
// returned); the distinct loops of the batch's records (three launches; pg_loops_ws_bytes: its workspace); what recognize leaves, for loop m
hipError_t launch_pg_recognize_all(const lsd_pg_head* head, int nodes_cap, const lsd_pg_desc* desc, lsd_pg_place_par par, int q_lo, int n_q,
                                   lsd_pg_place_rec* recs, lsd_pg_place_rep* reps, hipStream_t s);
size_t pg_loops_ws_bytes(int n_q, int k, int edges_cap);
void launch_pg_loops(const lsd_pg_place_rec* recs, const lsd_pg_place_rep* reps, int n_q, int k, const lsd_pg_head* head, const lsd_pg_edge* edges,
                     int edges_cap, lsd_pg_loops_par par, void* ws, lsd_pg_loop_rec* loops, lsd_pg_loops_rep* rep, hipStream_t s);
void launch_pg_loop_select(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_polar* store, const int* store_lens,
                           int store_stride, int gap, int window, const lsd_pg_loop_rec* loops, const lsd_pg_loops_rep* loops_rep, int m,
                           PgHandOver out, hipStream_t s);
// reduce (k_pgreduce.hip): a number of launches that nodes_cap fixes; pg_reduce_ws_bytes: its workspace (desc and rep may be null)
size_t pg_reduce_ws_bytes(int nodes_cap, int edges_cap, int store_stride);
void launch_pg_reduce(lsd_pg_head* head, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* tracks, int n_tracks,
                      lsd_polar* store, int* store_lens, int store_stride, lsd_pg_desc* desc, lsd_pg_reduce_par par, int32_t* map,
                      lsd_pg_reduce_rep* rep, void* ws, hipStream_t s);
void launch_dbgmath(int fn, const double* a, const double* b, double* o0, double* o1, size_t n, hipStream_t s);

// x86-64 cvttsd2si semantics of the reference's (int) casts: NaN, +-inf and
// out-of-range values give INT_MIN.  v_cvt_i32_f64 would give 0 / saturate instead.
__host__ __device__ inline int cvt_x86(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return (int)0x80000000;
    return (int)v;
}

}  // namespace lsdhip
