/*
 * lsd_hip.h -- C ABI of liblsdhip.so, the MI355X (gfx950) implementation of the LSD hot path of
 * Pyrokine/LineSegmentDetector-SLAM.
 *
 * The reference has no FFI layer: its boundary for this path is the C++ free function
 *     structLSD mylsd::myLineSegmentDetector(Mat MapGray, int oriMapCol, int oriMapRow,
 *                                            double sca, double sig, double angThre,
 *                                            double denThre, int pseBin);      LSD/myLSD.h:132
 * (definition LSD/myLSD.cpp:129-376), called from LSD/main_on_windows.cpp:70 and
 * LSD/main_on_linux.cpp:132.  Every entry point below states the reference interface it
 * replaces.  Plain pointers and sizes only; no C++/torch types; status codes, no exceptions.
 * The C++ adapter with the reference's own names lives in include/myLSD.h.
 *
 * There is NO CPU fallback: lsd_create() fails with LSD_ERR_NO_DEVICE when no gfx950 GPU is
 * visible, and nothing in this library computes the path on the host.
 */
#ifndef LSD_HIP_H
#define LSD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSD_ABI_VERSION 1

/* status codes */
enum {
    LSD_OK = 0,
    LSD_ERR_INVALID = 1,        /* bad argument */
    LSD_ERR_NO_DEVICE = 2,      /* no usable HIP device (the library never falls back to the CPU) */
    LSD_ERR_HIP = 3,            /* a HIP runtime call failed; see lsd_last_error() */
    LSD_ERR_UNSUPPORTED = 4,    /* parameter outside the implemented range (e.g. pseBin > 1024) */
    LSD_ERR_CAPACITY = 5,       /* more lines than max_lines in at least one image */
    LSD_ERR_NOMEM = 6,
    LSD_ERR_INTERNAL = 7        /* the region stage's watchdog gave an image up (a defect detector; lsd_last_error() names the image) */
};

/* The five LSD knobs of myLineSegmentDetector (LSD/myLSD.h:132); defaults LSD/baseFunc.h:64-68.
 * LSD_ERR_UNSUPPORTED, before anything is enqueued, if the tap radius exceeds 40 or K1's window (csrc/k1_lds.h) exceeds the device's LDS per workgroup: at sig = 0.6, sca >= 0.12 runs on 160 KiB. */
typedef struct lsd_params {
    double sca;      /* 0.3  */
    double sig;      /* 0.6  */
    double angThre;  /* 22.5 */
    double denThre;  /* 0.7  */
    int pseBin;      /* 1024 */
} lsd_params;

/* Layout-identical to structLinesInfo (LSD/baseFunc.h:33-44): 9 doubles + int, sizeof == 80. */
typedef struct lsd_line {
    double k, b, dx, dy, x1, y1, x2, y2, len;
    int orient;
} lsd_line;

typedef struct lsd_ctx lsd_ctx;

/* --- lifetime ------------------------------------------------------------------------ */
/* Creates a context bound to HIP device `device` (one context per GPU / per process rank). */
int lsd_create(lsd_ctx **out, int device);
void lsd_destroy(lsd_ctx *ctx);
const char *lsd_strerror(int status);
/* Text of the last HIP failure seen by this context ("" if none). */
const char *lsd_last_error(const lsd_ctx *ctx);
/* Fills the reference defaults (LSD/baseFunc.h:64-68). */
void lsd_default_params(lsd_params *p);
int lsd_abi_version(void);
/* Frees buffers returned through lines_out. */
void lsd_free(void *p);

/* --- the hot path, host buffers -------------------------------------------------------- */
/* Replaces mylsd::myLineSegmentDetector (LSD/myLSD.h:132, LSD/myLSD.cpp:129).
 *   map        IN-OUT rows x cols uint8, row pitch `stride` bytes.  As in the reference the
 *              caller's image is rewritten (1 -> 255, 255 -> 0 for y >= 1, x >= 1; myLSD.cpp:135-142).
 *   line_im    rows x cols uint8 (pitch line_im_stride), receives structLSD.lineIm (0/255), or NULL.
 *   lines_out  receives a malloc'ed array of *n_lines lsd_line (structLSD.linesInfo; free with lsd_free).
 * Blocking; uses the context's own streams.  Host buffers travel through pinned double buffers; the rewritten map comes
 * back while the rest of the pipeline still runs; the lines arrive compacted in one copy. */
int lsd_run(lsd_ctx *ctx, uint8_t *map, int cols, int rows, size_t stride, const lsd_params *p,
            uint8_t *line_im, size_t line_im_stride, lsd_line **lines_out, int *n_lines);

/* Batch of n equally sized images packed back to back (image i at maps + i*rows*cols, pitch cols).
 * offsets_out[n+1] receives the prefix sums of the per-image line counts; *lines_out the
 * concatenated lines (malloc'ed).  maps are rewritten like lsd_run does.  line_ims may be NULL. */
int lsd_run_batch(lsd_ctx *ctx, uint8_t *maps, int n, int cols, int rows, const lsd_params *p,
                  uint8_t *line_ims, lsd_line **lines_out, int *offsets_out);

/* Line capacity per image of the host entry points above (default 8192; the device entry point takes it as an argument).
 * An image with more lines returns its first max_lines and the call reports LSD_ERR_CAPACITY (lines_out is still valid). */
int lsd_set_host_max_lines(lsd_ctx *ctx, int max_lines);

/* --- the hot path, device-resident batch ------------------------------------------------ */
/* Same computation on buffers that already live in HBM (e.g. torch tensors' data_ptr()).
 *   d_maps     n x rows x cols uint8, read-only unless LSD_FLAG_WRITEBACK_MAP is set
 *   d_line_ims n x rows x cols uint8 or NULL
 *   d_lines    n x max_lines lsd_line (image i's lines start at d_lines + i*max_lines)
 *   d_counts   n int32 line counts.  A count > max_lines means that image overflowed (its first max_lines lines are valid; the
 *              host entry points report LSD_ERR_CAPACITY).  Nothing is written behind the first min(count, max_lines) records of an
 *              image, and the lineIm of an overflowing image holds the raster of its first max_lines lines only: the lines that
 *              were dropped leave no pixel (the reference has no capacity and marks them all).
 *              A count of -1 means the region stage's watchdog gave the image up
 *              (no wavefront of its workgroup found anything to do for seconds: a defect of the commit protocol, never seen
 *              on a released build): the image has no valid lines, its lineIm is blank, the other images are unaffected;
 *              the host entry points report LSD_ERR_INTERNAL and treat the image as having no lines.
 *   stream     hipStream_t on which to enqueue (NULL = the default stream, as everywhere in HIP).  Asynchronous:
 *              returns after enqueueing; workspace is (re)allocated before the first launch only
 *              when (n, cols, rows) grew. */
#define LSD_FLAG_WRITEBACK_MAP 1u
/* Known cliff: the wavefronts of an image's workgroup evaluate different seeds; ONE region's frontier is walked by one wavefront.  An
 * image made of regions of ten thousand pixels and more (sawtooth test images) returns the reference's result but takes 35-93 ms,
 * 2.8-3.3 x ONE host thread of the algorithm (measured: profiles/r06g_cliff_probe.log), where occupancy maps (largest region of the
 * reference's maps: 680 pixels) run hundreds of times faster than that thread in batches.  lsd_last_region_cycles shows it: occupancy
 * maps cost 57-350 cycles per scaled pixel, such images 850-1000. */
int lsd_enqueue_batch_device(lsd_ctx *ctx, uint8_t *d_maps, int n, int cols, int rows,
                             const lsd_params *p, unsigned flags, uint8_t *d_line_ims,
                             lsd_line *d_lines, int max_lines, int32_t *d_counts, void *stream);
/* Pre-sizes the workspace so that lsd_enqueue_batch_device never allocates: 103 B per scaled pixel on 4 wavefronts per image, 146 B on
 * 8 (lsd_set_region_waves, below; call it first), i.e. 39 / 55 MB per 2048 x 2048 map at sca 0.3 -- 20.0 / 28.2 GB for 512 of them
 * (tools/workspace_size.py).  The workspace is sized for the helper pool of the default help setting even while help is off, so that
 * lsd_set_region_help never makes a later enqueue allocate.  The lookup tables are sized here as well (log-gamma of every pixel count of
 * this geometry, the Gaussian taps of the DEFAULT parameters): an enqueue of a larger geometry than any reserved one still grows them
 * (one synchronisation, one allocation), an enqueue with other parameters rewrites the small ones (blocking copies, no allocation). */
int lsd_reserve(lsd_ctx *ctx, int n, int cols, int rows);
/* Blocks until the stream used by the last enqueue is idle. */
int lsd_synchronize(lsd_ctx *ctx);

/* --- multi-GPU: image shards and the hand-off of the line lists (BASELINE configs[4]) ------------------------- */
/* The reference runs one map on one host (LSD/main_on_windows.cpp:67-70, LSD/main_on_linux.cpp:130-132); a batch of independent
 * maps is sharded over the GPUs of a node, one process (or thread) and one lsd_ctx per GPU, with no collective on the data path.
 * The only exchange is the result hand-off below.
 * lsd_shard_range: the contiguous shard [*lo, *hi) of n_items images that rank `rank` of `world` takes. */
void lsd_shard_range(int n_items, int world, int rank, int *lo, int *hi);
/* Cost-aware deal of the same shards: perm[n_items] orders the images such that rank r, taking perm[lo_r .. hi_r) (lsd_shard_range),
 * carries about the same total cost as every other rank (longest-processing-time-first, deterministic; inside a shard ascending image
 * index).  costs[i] >= 0: e.g. the region stage's cycles of image i in the previous step (lsd_last_region_cycles) -- maps of one site
 * cost about the same from step to step.  The gathered lists then arrive in perm order: image perm[g] at position g. */
int lsd_shard_balanced(const long long *costs, int n_items, int world, int *perm);
/* Shader clocks the region stage spent on each of the first n images of the context's last batch (synchronises): the cost
 * lsd_shard_balanced deals by.  An image the region stage gave up reports 0.  LSD_ERR_INVALID if the context's last call did not run
 * the region stage on at least n images (lsd_set_stop_after). */
int lsd_last_region_cycles(lsd_ctx *ctx, int n, long long *cycles_out);

/* How much of the last batch's result hangs on the last place of the libm.  The reference decides with glibc's sin / cos / atan2 / exp /
 * log10 / pow (growth test LSD/myLSD.cpp:540-543, orientation flip :655-665, density :829 / :869, Refiner's width test :845, Reducer's
 * radius test :780, rectangle edges against pixel rows :973-1004, aligned count :1009-1013, RectangleImprover's comparisons of logNFA
 * :1075-1156, the "pi -> 0" rule :170); this library evaluates the same functions correctly rounded, and glibc's results are within
 * one ulp of those.  near_ties[i] = the number of decisions image i's evaluations took with their operands closer than that ulp can
 * move them (speculative evaluations included: an upper bound).  0: any libm within one ulp of correct rounding gives the same
 * decisions -- the lines, usedMap and lineIm of image i are the reference's on every such platform.  > 0: on this image a platform's
 * libm may decide (about one random map in 4 000 differs from the glibc build in one decision; each of those has
 * a count > 0 -- the property tools/campaign.py checks on every image).  Synchronises; LSD_ERR_INVALID if the last call did not run the
 * region stage on at least n images. */
int lsd_last_sensitivity(lsd_ctx *ctx, int n, int *near_ties);

/* A communicator as this library sees it: who am I, how many are we, and ONE operation -- an all-gather of equally sized device
 * buffers (d_recv holds world x bytes_per_rank, rank r's bytes at r * bytes_per_rank), enqueued on `stream`, 0 on success. */
typedef struct lsd_comm {
    int rank, world;
    int (*all_gather)(void *user, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
    void *user;
} lsd_comm;
/* Binds *out to an RCCL communicator (an ncclComm_t, passed as void*): rank / world from ncclCommUserRank / ncclCommCount,
 * all_gather = ncclAllGather(..., ncclInt8, comm, stream) -- RCCL over xGMI between the GPUs of a node.  The RCCL symbols are taken
 * from the RCCL the calling process has loaded (the library the communicator belongs to; a second copy is never loaded);
 * LSD_ERR_UNSUPPORTED if the process has none. */
int lsd_comm_from_rccl(void *nccl_comm, lsd_comm *out);

/* Sizes of the gathered arrays: *per_rank = images of the largest shard; *counts_words = world * (per_rank + 2) int32. */
int lsd_gather_layout(int n_total, int world, int *per_rank, size_t *counts_words);

/* Hands this rank's line lists to every rank.  d_lines / d_counts: the outputs of lsd_enqueue_batch_device for this rank's shard
 * (n_local == the size lsd_shard_range gives comm->rank, else LSD_ERR_INVALID).  On `stream`, without host synchronisation:
 *   1. the records are packed on the device, image-major, into a slab of cap_rows records (rows past the rank's lines are zero);
 *   2. all-gather of the padded counts:  d_counts_all [world][per_rank + 2] int32 -- rank r's per-image counts (clamped to
 *      max_lines, zero-padded), then [per_rank] = rows in its slab, [per_rank + 1] = flags: bit 0 it had to drop rows (more than
 *      cap_rows lines or an image over max_lines), bit 1 an image the region stage gave up (lsd_gather_unpack: LSD_ERR_CAPACITY
 *      resp. LSD_ERR_INTERNAL, with everything that did arrive in its outputs; LSD_ERR_INTERNAL outranks LSD_ERR_CAPACITY).  The torch
 *      packer of the Python package (dist.pack_lines) builds the same slab and the same clamped counts but folds both bits into one
 *      bool, over == (flags != 0): the two-bit word exists in this ABI only;
 *   3. all-gather of the slabs:          d_slabs_all [world][cap_rows] lsd_line.
 * Image g of the batch (rank r = its shard, local index j) has its lines at d_slabs_all[r][sum of counts[r][0..j)].
 * ~22 MB per GPU and step for the 512 x 2048^2 bench batch at cap_rows = 512 per image.
 * The packing stages through buffers of the CONTEXT: like lsd_enqueue_batch_device, one context serves one stream at a time -- a
 * second hand-off from the same context is ordered behind the first one's collectives (an event), whatever its stream. */
int lsd_gather_lines(lsd_ctx *ctx, const lsd_comm *comm, const lsd_line *d_lines, const int32_t *d_counts, int n_local, int max_lines,
                     int n_total, int cap_rows, int32_t *d_counts_all, lsd_line *d_slabs_all, void *stream);
/* Host side of the hand-off: turns HOST copies of the two gathered arrays into offsets_out[n_total + 1] and (if lines_out is
 * not NULL) the lines of all images in global image order (lines_cap records available; LSD_ERR_INVALID if more arrive).
 * LSD_ERR_CAPACITY if a rank flagged dropped rows (flag bit 0), LSD_ERR_INTERNAL if one flagged an image given up (bit 1; it
 * outranks the other); what arrived is still unpacked: the images of a rank from its slab's cut on are shorter by what it dropped. */
int lsd_gather_unpack(const int32_t *counts_all, const lsd_line *slabs_all, int n_total, int world, int cap_rows, int32_t *offsets_out,
                      lsd_line *lines_out, size_t lines_cap);

/* --- createMapCache (SURVEY 8f "next" #1) ------------------------------------------------------ */
/* Replaces mylsd::createMapCache(Mat MapGray, double res) (LSD/myLSD.h:131, LSD/myLSD.cpp:11-127): distance (metres)
 * from every cell to the occupied cell (value 1) whose breadth-first flood reaches it first, capped at
 * z_occ_max_dis (LSD/baseFunc.h:60; unreachable cells hold z_occ_max_dis, occupied cells 0).
 *   map  rows x cols uint8 (pitch `stride`), read-only -- call it BEFORE lsd_run, which rewrites the map (Q2);
 *   out  rows x cols doubles, packed (the CV_64FC1 mapCache FeatureAssociation reads, LSD/myFA.cpp:371-380).
 * Bit-identical to the reference (integer flood order + one exactly rounded sqrt and multiply per cell). */
int lsd_map_cache(lsd_ctx *ctx, const uint8_t *map, int cols, int rows, size_t stride, double res,
                  double z_occ_max_dis, double *out);
/* The same for n packed device-resident maps (d_out: n x rows x cols doubles), asynchronous on `stream`. */
int lsd_enqueue_map_cache_device(lsd_ctx *ctx, const uint8_t *d_maps, int n, int cols, int rows, double res,
                                 double z_occ_max_dis, double *d_out, void *stream);

/* --- scan-to-map matching batch (SURVEY 8f "next" #2) ------------------------------------------- */
/* Replaces the body of myfa::thread_ScanToMapMatch (LSD/myFA.cpp:197-270) with NormalizedLineDirection (:272-305),
 * rotateScanIm (:307-357) and CalcScore (:359-396), which the reference runs once per (map line, scan line) pair on a
 * 30-thread pool.  For pair p = {cntMapLine, cntScanLine} and matching i = 1..4 (:205-249)
 *   out[4 * p + i - 1] = { rotated lidar pose (x, y, angDiff in (-180, 180]), score }
 * with score = INFINITY where rotateScanIm rejects the candidate (farther than max_esti_dist from last_pose, :330) or
 * CalcScore does (:388).  The caller keeps score < 3 and sorts, as FeatureAssociation does (:60-100).
 * lsd_position == structPosition (LSD/baseFunc.h:46-50); lines are structLinesInfo; map_cache is the rows x cols
 * CV_64FC1 array of lsd_map_cache.  Scores agree with the reference arithmetic up to the libm caveat of lsd_run. */
typedef struct lsd_position { double x, y, ang; } lsd_position;
typedef struct lsd_match_score { lsd_position pos; double score; } lsd_match_score;
int lsd_scan_to_map_match(lsd_ctx *ctx, const double *map_cache, int cols, int rows,
                          const lsd_line *map_lines, int n_map, const lsd_line *scan_lines, int n_scan,
                          const lsd_position *scan_im_points, int n_points, lsd_position lidar_pose, lsd_position last_pose,
                          const int *pairs, int n_pairs, double z_occ_max_dis, double max_esti_dist, lsd_match_score *out);
/* The same with every array resident on the device (d_map_cache as written by lsd_enqueue_map_cache_device), asynchronous
 * on `stream`; pair indices are NOT range-checked here. */
int lsd_enqueue_scan_to_map_match_device(lsd_ctx *ctx, const double *d_map_cache, int cols, int rows,
                                         const lsd_line *d_map_lines, const lsd_line *d_scan_lines,
                                         const lsd_position *d_scan_im_points, int n_points, lsd_position lidar_pose,
                                         lsd_position last_pose, const int *d_pairs, int n_pairs, double z_occ_max_dis,
                                         double max_esti_dist, lsd_match_score *d_out, void *stream);

/* --- scan-line extraction batch (SURVEY 8f "next" #4) ------------------------------------------- */
/* Replaces myrdp::FeatureScan (LSD/myRDP.cpp:9-185; RegionSegmentation :274-345, SplitMerge / SplitMergeAssistant :187-272,
 * getThresholdDeltaDist :347-368; caller LSD/main_on_windows.cpp:127) for a BATCH of lidar scans: n_scans scans at a pitch of
 * `stride` readings, scan i holding lens[i] <= stride finite readings (range, angle) -- what the caller's read loop leaves
 * after dropping the infinite ranges (:115-121).  Per scan i:
 *   lines_out[i * 360 .. ]   the line records (structLinesInfo) in the reference's order; n_lines[i] is their number, of which the
 *                            first 360 are stored (the reference's malloc, :39, which it would overrun: the host entry point returns
 *                            LSD_ERR_CAPACITY when a scan has more, the stored records are valid)
 *   pts_out[i * pts_cap .. ] scanImPoint: the pixels of the lines' rasters (x, y, 0) in the reference's order; n_pts[i] is
 *                            their number, of which the first pts_cap are stored
 *   lidar_pos[2 i .. ]       structLidarPointRec lidarPos (x, y), :33-36;  im_size[2 i ..] = (cols, rows) of FS.lineIm, :31
 * FS.lineIm itself is im_size zeros with 255 at the listed pixels.  region_point_limit / thre_line / line_dist_thre_m are
 * rdp_leastPoint / rdp_threLine / rdp_leastDist (LSD/baseFunc.h:70-72: 3, 0.08, 0.5).  lens[i] <= stride <= the context's scan
 * capacity (lsd_set_scan_capacity: 1024 unless raised); a larger stride is LSD_ERR_UNSUPPORTED.
 * lsd_polar is structLidarPointPolar (LSD/myRDP.h:34-38) without its `split` work flag; lsd_map_param is structMapParam
 * (LSD/baseFunc.h:25-31). */
typedef struct lsd_polar { double range, angle; } lsd_polar;
typedef struct lsd_map_param { int oriMapCol, oriMapRow; double mapResol, mapOriX, mapOriY; } lsd_map_param;
#define LSD_RDP_MAX_LINES 360
/* The scan capacity of a context: the most readings per scan (the largest `stride`) that FeatureScan, the two ingest entries and
 * lsd_localize take.  1024 by default -- the reference's lidar has 360 --; a context for a lidar with more readings per revolution
 * (1081, 1141, 3200 ...) raises it, up to LSD_SCAN_MAX_LEN.  Strides above 1024 run on a kernel of their own whose LDS grows with
 * the launch's stride, not with the capacity (26 bytes per reading: 104 KiB at 4096), with the same results bit for bit; strides up
 * to 1024 run as before whatever the capacity.  The line records stay LSD_RDP_MAX_LINES per scan: a long scan with more chords
 * reports the full count, stores the first 360, and the host entry points return LSD_ERR_CAPACITY.
 * lsd_set_scan_capacity: LSD_ERR_INVALID below 1024, LSD_ERR_UNSUPPORTED above LSD_SCAN_MAX_LEN or where a scan of `readings`
 * would need more LDS than the device gives a workgroup (lsd_last_error says how much).  Nothing is enqueued or allocated. */
#define LSD_SCAN_MAX_LEN 4096
int lsd_set_scan_capacity(lsd_ctx *ctx, int readings);
int lsd_scan_capacity(const lsd_ctx *ctx);
int lsd_feature_scan_batch(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, lsd_map_param map_param,
                           int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line *lines_out, int *n_lines,
                           lsd_position *pts_out, int pts_cap, int *n_pts, double *lidar_pos, int *im_size);
/* The same with every array resident on the device, asynchronous on `stream`.  The running time grows with the pixel extent of a
 * scan (the raster loops take one step per pixel of a line's extent, in one lane): the caller bounds the ranges. */
int lsd_enqueue_feature_scan_batch_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                          lsd_map_param map_param, int region_point_limit, double thre_line, double line_dist_thre_m,
                                          lsd_line *d_lines_out, int *d_n_lines, lsd_position *d_pts_out, int pts_cap, int *d_n_pts,
                                          double *d_lidar_pos, int *d_im_size, void *stream);

/* --- Scan ingestion: the drivers' read loop on the device ------------------------------------------ */
/* Replaces the loop in front of FeatureScan that drops the readings with an infinite range and packs the rest to the front of
 * lidarPointPolar[] (the file driver, LSD/main_on_windows.cpp:104-123; laserCallback, LSD/main_on_linux.cpp:53-66), for a BATCH of
 * raw scans resident on the device: one launch (k_ingest.hip), asynchronous on `stream`, no workspace, no synchronisation.  It writes
 * exactly what lsd_enqueue_feature_scan_batch_device reads: d_scans (n_scans x stride readings: the kept ones first, in beam order,
 * then EVERY slot from d_lens[i] to stride as +0.0 / +0.0) and d_lens (n_scans ints).  1 <= n_beams <= stride <= the context's scan
 * capacity (lsd_set_scan_capacity; 1024 by default).
 *   d_raw    n_scans x n_beams (range, angle) pairs, the file driver's layout (Lidar.txt).  A reading is kept iff `range != INFINITY`
 *            as the reference evaluates it (:115): -inf and NaN are KEPT, only +inf is dropped.
 *   d_take   optional (NULL: every scan is taken), one int per scan: where it is 0 the scan has d_lens[i] = 0 and an all-zero row.
 * d_raw and d_scans must not overlap (in-place is not supported) and must be 16-byte aligned (every hipMalloc'ed or torch base is).
 * LSD_ERR_INVALID on a null or non-positive argument, n_beams > stride or a misaligned pointer; LSD_ERR_UNSUPPORTED on a stride above
 * the scan capacity. */
int lsd_enqueue_scan_ingest_device(lsd_ctx *ctx, const lsd_polar *d_raw, int n_scans, int n_beams, const int *d_take,
                                   lsd_polar *d_scans, int *d_lens, int stride, void *stream);
/* The same from sensor_msgs/LaserScan fields: d_ranges (n_scans x n_beams floats) and d_angle_min_inc (n_scans x 2 floats:
 * angle_min, angle_increment of each message).  Kept iff `ranges[i] != INFINITY` in float (:57); range = (double)ranges[i];
 * angle = (double)(angle_min + i * angle_increment) as the callback writes it on float fields (:60): the product and the sum are each
 * rounded to SINGLE precision, never fused.
 * NOT reproduced: laserCallback stores a finite reading at lidarPointPolar[i], not [len_lp], and then hands the first len_lp entries to
 * FeatureScan, so with any infinite range it reads stale entries of earlier messages.  The file driver packs, and so do both entries. */
int lsd_enqueue_laserscan_ingest_device(lsd_ctx *ctx, const float *d_ranges, const float *d_angle_min_inc, int n_scans, int n_beams,
                                        const int *d_take, lsd_polar *d_scans, int *d_lens, int stride, void *stream);

/* --- FeatureAssociation: pose fusion, UKF update and log replay ----------------------------------- */
/* Replaces myfa::FeatureAssociation (LSD/myFA.cpp:13-184) with myfa::ukf (:404-536), and the frame loop of the replay driver
 * (LSD/main_on_windows.cpp:80-186).  Per frame: the pair list of :28-58 (scan lines of len >= 40 against map lines within 35 % of
 * their length, in that loop order), four scored candidates per pair (lsd_scan_to_map_match), those with score < 3 kept in
 * single-thread order and sorted stably by score, then one of three branches:
 *   LSD_FA_RESET  nothing kept: x = (-1, -1, 0, ...), P = diag(100, 100, 100, 1, 1, 1, .1, .1, .1)                 (:62-83)
 *   LSD_FA_FIRST  |lastPose.x + 1| < 1e-4: x = the input x with x[0..2] = the best candidate's pose, P unchanged        (:86-95)
 *   LSD_FA_UKF    weighted mean of the kept poses (w = 1/score^2), then the 9-state unscented update                (:140-176)
 * The arithmetic is the reference's in its statement order, without FMA; the Eigen calls are restated as Eigen's own algorithms
 * (unblocked LLT, the 3x3 cofactor inverse, ascending sums) -- bitwise agreement with an Eigen build is NOT verified.
 * Quirks kept: the sigma points take ROWS of L (:446), a kept score of 0 makes the state NaN, a P that is not positive definite is
 * factored up to its first failing column, angles are averaged without wrapping. */
typedef struct lsd_fa_state {
    double x[9];     /* kalman_x */
    double P[81];    /* kalman_P, column-major as Eigen stores it (kalman_P.data()) */
} lsd_fa_state;
enum { LSD_FA_RESET = 0, LSD_FA_FIRST = 1, LSD_FA_UKF = 2 };
typedef struct lsd_fa_report {
    lsd_position estimate;   /* poseEstimate: the fused pose (UKF), the best candidate (FIRST), (-1, -1, 0) (RESET) */
    double score;            /* its score (1/sqrt(sum w / n), the candidate's, INFINITY) */
    lsd_position scan_pose;  /* the ScanPose the frame used */
    int n_pairs;             /* pairs scored (4 candidates each) */
    int n_kept;              /* candidates with score < 3 */
    int branch;              /* LSD_FA_* */
    int llt;                 /* UKF branch: -1 if LLT(P) succeeded, else the first column it stopped at; -2 on the other branches */
} lsd_fa_report;
/* The driver's starting state (LSD/main_on_windows.cpp:80-93): x = (-1, -1, 0, ...), P = diag(100, 100, 100, 1, 1, 1, .1, .1, .1). */
void lsd_fa_initial_state(lsd_fa_state *out);
/* One frame from host buffers: the drop-in for myfa::FeatureAssociation(&FAInput).  The FAInput fields are the arguments:
 * map_cache (rows x cols), map lines, scan lines, scanImPoint, lidarPose (rounded on the device as trans2FA does, :228-229),
 * lastPose, ScanPose and the state in; the state out (FAOutput.kalman_x / kalman_P) and the report.  in and out may alias.
 * Blocking. */
int lsd_feature_association(lsd_ctx *ctx, const double *map_cache, int cols, int rows, const lsd_line *map_lines, int n_map,
                            const lsd_line *scan_lines, int n_scan, const lsd_position *scan_im_points, int n_points,
                            lsd_position lidar_pose, lsd_position last_pose, lsd_position scan_pose, const lsd_fa_state *in,
                            lsd_fa_state *out, lsd_fa_report *report);
/* The replay loop for n_seq independent sequences against ONE map, on the device, asynchronous on `stream` (no host
 * synchronisation between frames; 3 launches per frame index).  Frame t of sequence s uses slot s * frames_pitch + t of the
 * lsd_enqueue_feature_scan_batch_device outputs (d_lines at slot * LSD_RDP_MAX_LINES, d_pts at slot * pts_cap; at most 360
 * lines and pts_cap points of a scan are used), for t < n_frames[s] (a HOST array: the sequences are ragged).  d_odom holds
 * n_seq x (frames_pitch + 1) odometry rows: the reference's Odom vector of the sequence (Odom[0].x = 0, frame t uses rows t and
 * t + 1).  Per frame: ScanPose from the odometry and the mean of the past angle offsets (:125-140), lastPose = the previous state's
 * x[0..2] (the initial state's at t = 0), FeatureAssociation, then the offset bookkeeping of :170-180.  d_states / d_reports:
 * n_seq x frames_pitch records (slots past a sequence's end are not written).  The context's workspace grows before the first
 * launch when needed (one synchronisation).
 * d_init: each sequence starts at the driver's FIRST frame (cnt_frame = 1): the past angle offsets start empty, so an initial state
 * must be a reset one (x[0] = -1, e.g. lsd_fa_initial_state) -- resuming a sequence midway from a state with x[0] != -1 would take the
 * mean of no offsets (0/0) as the reference would, and its ScanPose, hence the whole trajectory, becomes NaN.  To continue a sequence
 * across calls (a live robot, a checkpoint), use lsd_enqueue_localize_resume_device, which carries the loop's variables.
 * Pairs, candidates and the loop's bookkeeping live in the CONTEXT's workspace: like lsd_enqueue_batch_device, one context serves
 * one stream at a time -- another FeatureAssociation call on the same context (any stream) must not start before this one has
 * finished (synchronise the stream, or use one context per stream). */
int lsd_enqueue_localize_device(lsd_ctx *ctx, const double *d_map_cache, int cols, int rows, const lsd_line *d_map_lines, int n_map,
                                int n_seq, int frames_pitch, const int *n_frames, const lsd_line *d_lines, const int *d_n_lines,
                                const lsd_position *d_pts, int pts_cap, const int *d_n_pts, const double *d_lidar_pos,
                                const lsd_position *d_odom, double map_resol, const lsd_fa_state *d_init, lsd_fa_state *d_states,
                                lsd_fa_report *d_reports, void *stream);
/* The replay driver's loop variables after some number of frames (LSD/main_on_windows.cpp:80-180), per sequence: what
 * lsd_enqueue_localize_resume_device reads before a sequence's first frame of a call and writes after its last.  Plain bytes: a caller
 * may copy it, keep it on the host, write it to disk and resume later. */
typedef struct lsd_fa_carry {
    lsd_fa_state state;   /* kalman_x / kalman_P after the last frame; lastPose = state.x[0..2] */
    lsd_position odom;    /* Odom[cnt_frame]: the odometry row the last frame used as its new row (initially Odom[0]) */
    double ang_sum;       /* the sum of angRotate, accumulated from 0 in push order (the reference's theta loop re-sums it so) */
    double ang_count;     /* angRotate.size() */
    int32_t frames;       /* cnt_frame: frames consumed so far (0: the next frame is the driver's first) */
    int32_t is_offset;    /* isOffset (0 / 1) */
} lsd_fa_carry;           /* 768 bytes */
/* A carry before the driver's first frame: state (NULL: lsd_fa_initial_state), odom0 = Odom[0] (the driver sets Odom[0].x = 0),
 * empty angle offsets, frames = 0, is_offset = 0. */
void lsd_fa_carry_init(lsd_fa_carry *out, const lsd_fa_state *state, lsd_position odom0);
/* The replay loop of lsd_enqueue_localize_device, resumable: each sequence continues from its carry d_carry[s] (device, n_seq records,
 * read and updated in place).  Frame t (t < n_frames[s], a HOST array) of sequence s uses slot s * frames_pitch + t of the FeatureScan
 * outputs and of d_states / d_reports, as there.  d_odom holds n_seq x frames_pitch rows: row t is the NEW odometry row of frame t,
 * Odom[cnt_frame]; Odom[cnt_frame - 1] is the carry's odom at t = 0, else row t - 1.  The carry supplies lastPose and the previous
 * state, the running sum and count of angRotate and isOffset, and cnt_frame (so the cnt_frame == 1 test of :176 is the sequence's
 * global first frame, not the call's).  After the call d_carry[s] holds the driver's variables after that sequence's last frame; a
 * sequence with n_frames[s] == 0 keeps its carry bit for bit and none of its state or report slots is written.  Splitting a sequence
 * into calls at any frame gives the same states and reports, bit for bit, as one call from lsd_fa_carry_init.
 * Like lsd_enqueue_localize_device: pairs and candidates live in the CONTEXT's workspace, so one context serves one stream at a time
 * (synchronise before another FeatureAssociation call on the same context, or use one context per stream); the workspace grows
 * before the first launch when needed (one synchronisation).  LSD_ERR_INVALID for a null carry, n_frames[s] outside 0..frames_pitch
 * and the argument errors of lsd_enqueue_localize_device. */
int lsd_enqueue_localize_resume_device(lsd_ctx *ctx, const double *d_map_cache, int cols, int rows, const lsd_line *d_map_lines,
                                       int n_map, int n_seq, int frames_pitch, const int *n_frames, const lsd_line *d_lines,
                                       const int *d_n_lines, const lsd_position *d_pts, int pts_cap, const int *d_n_pts,
                                       const double *d_lidar_pos, const lsd_position *d_odom, double map_resol, lsd_fa_carry *d_carry,
                                       lsd_fa_state *d_states, lsd_fa_report *d_reports, void *stream);
/* The two loops above against a map that is still being made when the call is enqueued (lsd_enqueue_map_update_device on an earlier
 * stream position): the map's line count is read ON THE DEVICE, by the one kernel that uses it (the pair list of :28-58), as
 * min(max(*d_n_map, 0), map_lines_cap) -- the detector's count conventions: an overflowed count leaves the first map_lines_cap records
 * valid, -1 (an image given up) none.  d_map_lines holds map_lines_cap records.  Everything the host sizes -- the context's workspace,
 * the limit map_lines_cap * 360 <= 1 << 26 (LSD_ERR_UNSUPPORTED) -- is sized from map_lines_cap as the entries above size it from
 * n_map; every other argument and rule is theirs.  LSD_ERR_INVALID also for a null d_n_map or map_lines_cap <= 0.  With *d_n_map ==
 * n_map <= map_lines_cap the states and reports are those of the entries above, bit for bit. */
int lsd_enqueue_localize_live_map_device(lsd_ctx *ctx, const double *d_map_cache, int cols, int rows, const lsd_line *d_map_lines,
                                         int map_lines_cap, const int32_t *d_n_map, int n_seq, int frames_pitch, const int *n_frames,
                                         const lsd_line *d_lines, const int *d_n_lines, const lsd_position *d_pts, int pts_cap,
                                         const int *d_n_pts, const double *d_lidar_pos, const lsd_position *d_odom, double map_resol,
                                         const lsd_fa_state *d_init, lsd_fa_state *d_states, lsd_fa_report *d_reports, void *stream);
int lsd_enqueue_localize_resume_live_map_device(lsd_ctx *ctx, const double *d_map_cache, int cols, int rows, const lsd_line *d_map_lines,
                                                int map_lines_cap, const int32_t *d_n_map, int n_seq, int frames_pitch, const int *n_frames,
                                                const lsd_line *d_lines, const int *d_n_lines, const lsd_position *d_pts, int pts_cap,
                                                const int *d_n_pts, const double *d_lidar_pos, const lsd_position *d_odom, double map_resol,
                                                lsd_fa_carry *d_carry, lsd_fa_state *d_states, lsd_fa_report *d_reports, void *stream);
/* A fleet on several maps in one call.  lsd_map_ref describes one device-resident map: what the entries above take as d_map_cache,
 * cols, rows, d_map_lines, n_map (and d_n_map: NULL, or the live-map convention above with n_map as the capacity) and, from
 * lsd_map_param, the three values FeatureScan and the loop read.  The table maps[n_maps] is a HOST array (as n_frames is): every field
 * is checked on the host, and the entry copies it to the device from context-owned storage without waiting for the stream.  d_map_of is
 * a DEVICE array of one int32 per sequence: the map id of sequence s, read when the kernels run, so re-assigning a robot is a device
 * write.  An id outside 0..n_maps-1 (use -1) means the sequence sits the call out: its carry, its state and report slots keep their
 * bytes, it counts no pairs and no candidates, FeatureScan writes counts 0 for its scans and nothing else, and no other sequence is
 * affected.
 *   lsd_enqueue_feature_scan_maps_device      lsd_enqueue_feature_scan_batch_device with mapResol / mapOriX / mapOriY of scan i taken
 *                                             from map d_map_of[i / scans_per_seq] (the Localizer's slot layout: slot = s * k + t)
 *   lsd_enqueue_localize_maps_device          lsd_enqueue_localize_device, sequence s against map d_map_of[s]
 *   lsd_enqueue_localize_resume_maps_device   lsd_enqueue_localize_resume_device, likewise
 * Every sequence gets, bit for bit, what it gets alone on its map through those entries.  The per-sequence workspace and the pair limit
 * (LSD_ERR_UNSUPPORTED) are taken from the largest n_map of the table.  Refused before anything is enqueued: LSD_ERR_INVALID for
 * n_maps <= 0, a null table, a null d_map_of, scans_per_seq <= 0, a map with cols or rows <= 0, n_map < 0, a null cache, null lines at
 * n_map > 0 or mapResol not > 0 (and the argument errors of the entries above); LSD_ERR_UNSUPPORTED for n_maps > LSD_MAX_MAPS. */
#define LSD_MAX_MAPS 64
typedef struct lsd_map_ref {
    const double   *d_map_cache;   /* rows x cols */
    const lsd_line *d_map_lines;   /* n_map records (capacity when d_n_map is set) */
    const int32_t  *d_n_map;       /* NULL: n_map is the count; else the count is read on the device and held to 0..n_map */
    int cols, rows, n_map;
    double mapResol, mapOriX, mapOriY;
} lsd_map_ref;
int lsd_enqueue_feature_scan_maps_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                         const lsd_map_ref *maps, int n_maps, const int32_t *d_map_of, int scans_per_seq,
                                         int region_point_limit, double thre_line, double line_dist_thre_m, lsd_line *d_lines_out,
                                         int *d_n_lines, lsd_position *d_pts_out, int pts_cap, int *d_n_pts, double *d_lidar_pos,
                                         int *d_im_size, void *stream);
int lsd_enqueue_localize_maps_device(lsd_ctx *ctx, const lsd_map_ref *maps, int n_maps, const int32_t *d_map_of, int n_seq,
                                     int frames_pitch, const int *n_frames, const lsd_line *d_lines, const int *d_n_lines,
                                     const lsd_position *d_pts, int pts_cap, const int *d_n_pts, const double *d_lidar_pos,
                                     const lsd_position *d_odom, const lsd_fa_state *d_init, lsd_fa_state *d_states,
                                     lsd_fa_report *d_reports, void *stream);
int lsd_enqueue_localize_resume_maps_device(lsd_ctx *ctx, const lsd_map_ref *maps, int n_maps, const int32_t *d_map_of, int n_seq,
                                            int frames_pitch, const int *n_frames, const lsd_line *d_lines, const int *d_n_lines,
                                            const lsd_position *d_pts, int pts_cap, const int *d_n_pts, const double *d_lidar_pos,
                                            const lsd_position *d_odom, lsd_fa_carry *d_carry, lsd_fa_state *d_states,
                                            lsd_fa_report *d_reports, void *stream);
/* Carries from one map frame to another.  A carry's state holds the pose, its velocity and its acceleration in PIXELS of the map it was
 * made on (FeatureScan and the loop turn metres into pixels with mapResol / mapOriX / mapOriY), so a map that comes back with another
 * origin or resolution -- a SLAM map that grew -- leaves lastPose off by the shift; the reference's node carries no state between scans
 * and never met this.  lsd_enqueue_fa_carry_rebase_device moves d_carry[0..n_seq) (device) from frame `from` to frame `to`, in place,
 * asynchronous on `stream`, in one launch, without workspace: it allocates nothing and waits for nothing.
 * Sequence s moves iff d_key is NULL or d_key[s] == key, read ON THE DEVICE when the kernel runs: with d_key = d_map_of it means "the
 * robots on map `key`" and stays right behind an earlier re-assignment on the stream.  Every other carry keeps its bytes.
 * Arithmetic, fp64 without FMA, in this order:  s = from.mapResol / to.mapResol;  tx = (from.mapOriX - to.mapOriX) / to.mapResol, ty
 * likewise;  x[0] = x[0] * s + tx, x[1] = x[1] * s + ty;  x[3], x[4], x[6], x[7] *= s;  x[2], x[5], x[8] (degrees) untouched;
 * P[i][j] = (P[i][j] * d_i) * d_j with d_k = s for k % 3 != 2, else 1;  odom (metres), ang_sum, ang_count, frames, is_offset untouched.
 * With equal resolutions s is exactly 1: P and the rates keep their bits, only x[0] and x[1] shift.  The pose in metres, x * mapResol +
 * mapOri, is preserved up to rounding; nothing about orientation is (the reference reads only origin.position).
 * Left alone, bit for bit: a carry without a pose, |x[0] + 1| < 1e-4 -- the reference's own "no pose yet / just reset" test
 * (myFA.cpp:99), which the exact lastPose.x == -1 of :330 would otherwise stop recognising.  A NaN state stays NaN by the arithmetic.
 * from == to in all three fields launches nothing and returns LSD_OK.  Refused before anything is enqueued, LSD_ERR_INVALID: a null
 * carry, n_seq <= 0, a resolution that is not finite and > 0, a non-finite origin. */
typedef struct lsd_map_frame { double mapResol, mapOriX, mapOriY; } lsd_map_frame;
int lsd_enqueue_fa_carry_rebase_device(lsd_ctx *ctx, lsd_fa_carry *d_carry, int n_seq, const int32_t *d_key, int32_t key,
                                       lsd_map_frame from, lsd_map_frame to, void *stream);
/* The grid match response fused into the carry: a measurement update of the carry's 9-state filter with a response record (the section
 * "the response around a match" below) as the measurement -- the filter's own closing lines (myfa::ukf: K = Pxz Pzz^-1, x += K Zdiff, P =
 * P1 - K Pxz^T) with H = [I3 0], so that the NEXT tick starts from the corrected lastPose (csrc/k_facorrect.hip; restated
 * in tests/fa_correct_cases.py).  In place on d_carry[0..n_seq), asynchronous on `stream`, one launch, no workspace, no atomics: it
 * allocates nothing and waits for nothing.  fp64 without FMA; every sum runs ascending from 0.0; P(i,j) = state.P[j * 9 + i].
 * Per sequence s: its carry, the frames_pitch ORIGINAL poses of its slots -- the first 24 bytes of the record at d_poses + (s *
 * frames_pitch + t) * pose_pitch, the poses the match was given (a Localizer's tick: its states, pitch 720) -- and the response records
 * d_resp[s * frames_pitch + t].  The first test that fires decides; each outcome is exactly one flag; report fields that were not
 * computed are +0.0 and slot is -1; the carry keeps every byte unless the outcome is APPLIED:
 *   0. d_key != NULL and d_key[s] != key, read ON THE DEVICE as the re-base reads it: nothing of s is written, carry or report
 *   1. fabs(x[0] + 1) < 0.0001, the "no pose yet" test of the re-base: NO_POSE
 *   2. any of the 90 doubles of the state not finite: NOT_FINITE
 *   3. slot = the LARGEST t in 0..frames_pitch-1 whose original pose's 24 bytes equal the 24 bytes of state.x[0..2] (bytes, not values:
 *      -0.0 is not +0.0); none: STALE.  The carry holds the state of the last frame the tick took and slots past n_frames hold zeroed
 *      states, so this finds that frame without n_frames, a host copy or a wait -- and refuses a carry that has moved on since the match
 *   4. r = d_resp[s * frames_pitch + slot]: VALID clear, or NONE, EMPTY or MISMATCH set: NO_RESPONSE (slot reported); r.x, r.y, r.ang or
 *      one of r.cov[0..5] not finite: NOT_FINITE (slot reported).  The *_NOT_PEAK bits stop nothing: the offset of such an axis is zero and
 *      its covariance weighs it
 *   5. R(0,0) = cov[0] * cov_scale + floor_xy, R(1,1) = cov[2] * cov_scale + floor_xy, R(2,2) = cov[5] * cov_scale + floor_ang, R(0,1) =
 *      R(1,0) = cov[1] * cov_scale, R(0,2) = R(2,0) = cov[3] * cov_scale, R(1,2) = R(2,1) = cov[4] * cov_scale;  S(r,q) = P(r,q) + R(r,q),
 *      r, q < 3 (P is not symmetrised);  cof(r,q) = S(r1,q1) * S(r2,q2) - S(r1,q2) * S(r2,q1) with cyclic indices;  det = (cof(0,0) *
 *      S(0,0) + cof(1,0) * S(1,0)) + cof(2,0) * S(2,0);  invdet = 1 / det;  Sinv(j,i) = cof(i,j) * invdet.  !(det > 0) or invdet not
 *      finite: SINGULAR (det, slot reported)
 *   6. innov[q] = z[q] - x[q], z = (r.x, r.y, r.ang), angles not wrapped;  t[i] = sum_j Sinv(i,j) * innov[j];  d2 = sum_i innov[i] * t[i].
 *      gate > 0 and !(d2 <= gate): GATED, a NaN d2 included (innov, d2, det, slot reported)
 *   7. APPLIED (innov, d2, det, slot reported):  K(i,q) = sum_{r<3} P(i,r) * Sinv(r,q), i < 9;  x'[i] = x[i] + sum_q K(i,q) * innov[q];
 *      P'(i,j) = P(i,j) - sum_{r<3} K(i,r) * P(j,r).  odom, ang_sum, ang_count, frames and is_offset keep their bytes: the next frame
 *      computes its own angle offset from the corrected x[2]
 * (A NaN that the arithmetic itself makes of finite inputs -- an overflow -- is reported with the sign and payload the hardware gives it.)
 * With frames_pitch > 1 only the response of the LAST frame taken is fused: the states of earlier frames are already consumed by the loop.
 * d_rep may be NULL.  Refused before anything is enqueued, LSD_ERR_INVALID, outputs untouched: a null ctx, d_carry, d_poses or d_resp;
 * n_seq <= 0; frames_pitch outside 1..4096; pose_pitch < 24 or not a multiple of 8; a pointer that is not 8-byte aligned (d_key: 4-byte);
 * one of the four parameters not finite or negative. */
typedef struct lsd_grid_response_rec lsd_grid_response_rec;
typedef struct lsd_fa_correct_par { double cov_scale, floor_xy, floor_ang, gate; } lsd_fa_correct_par;   /* 32 bytes */
typedef struct lsd_fa_correct_rep {                                                                       /* 48 bytes */
    double innov[3]; double d2; double det; int32_t slot; uint32_t flags;
} lsd_fa_correct_rep;
enum { LSD_FA_CORRECT_APPLIED = 1, LSD_FA_CORRECT_NO_POSE = 2, LSD_FA_CORRECT_NOT_FINITE = 4, LSD_FA_CORRECT_STALE = 8,
       LSD_FA_CORRECT_NO_RESPONSE = 16, LSD_FA_CORRECT_SINGULAR = 32, LSD_FA_CORRECT_GATED = 64 };
int lsd_enqueue_fa_carry_correct_device(lsd_ctx *ctx, lsd_fa_carry *d_carry, int n_seq, int frames_pitch, const void *d_poses,
                                        size_t pose_pitch, const lsd_grid_response_rec *d_resp, const int32_t *d_key, int32_t key,
                                        lsd_fa_correct_par par, lsd_fa_correct_rep *d_rep /* may be NULL */, void *stream);
/* Host convenience: carries (n_seq, updated in place), poses (n_seq x frames_pitch, packed), resp (n_seq x frames_pitch) and rep (n_seq,
 * may be NULL) are host arrays; every sequence takes part (no key).  Blocking. */
int lsd_fa_carry_correct(lsd_ctx *ctx, lsd_fa_carry *carries, int n_seq, int frames_pitch, const lsd_position *poses,
                         const lsd_grid_response_rec *resp, lsd_fa_correct_par par, lsd_fa_correct_rep *rep);
/* Relocalisation on the device: the robots whose tick left them without a pose are gathered, located on the grid (the section "global
 * scan-to-grid localisation" below, its entry unchanged) and their carries seeded with the located pose, all on the tick's stream
 * (csrc/k_falost.hip, csrc/k_faseed.hip; restated in tests/fa_relocate_cases.py).
 * lsd_enqueue_fa_lost_gather_device picks the lost sequences of a tick and packs their scans into a batch of max_lost rows: what
 * lsd_enqueue_grid_locate_device takes with n_scans = max_lost, so that its launches and its workspace follow max_lost and not the fleet.
 * d_carry[n_seq], d_poses / pose_pitch (the tick's states, pitch 720) and d_key / key are the correction's; d_scans / d_lens / stride are
 * the tick's ingested scans, slot s * frames_pitch + t.  Sequence s is LOST iff all of these hold:
 *   - d_key is NULL or d_key[s] == key, read ON THE DEVICE as the re-base reads it
 *   - fabs(x[0] + 1) < 0.0001, the "no pose" test of the re-base (a NaN x[0] is not lost)
 *   - a slot exists: the LARGEST t in 0..frames_pitch-1 whose original pose's 24 bytes equal the 24 bytes of state.x[0..2] (the
 *     correction's step 3: bytes, not values) AND whose d_lens[s * frames_pitch + t] > 0 -- the frame had a scan.  A lost robot whose tick
 *     took no frame, or only empty scans, has no slot and is not gathered
 * The lost sequences take the ranks j = 0, 1, .. in ASCENDING s (a fleet with more lost robots than max_lost serves the lowest indices
 * first; rotating the start is the caller's).  For j < max_lost: d_pick[j] = s * frames_pitch + slot, row j of d_scans_out is that slot's
 * `stride` readings byte for byte, d_lens_out[j] its length.  For the rows at and past the number gathered: d_lens_out[j] = 0 (the locate
 * entry ends such a row in LSD_GRID_LOCATE_EMPTY without a search), d_pick[j] = -1, and the scan row keeps its bytes.  d_n_lost[0] = the
 * number of lost sequences, exact, possibly above max_lost; d_n_lost[1] = min(d_n_lost[0], max_lost).
 * Asynchronous on `stream`, ONE launch of min(max_lost, 128) workgroups whatever the data, no workspace, no atomics (the ranks are a
 * ballot / mbcnt prefix count in one pass over n_seq, made by every workgroup for the ranks it copies), no allocation and no wait.  The
 * slot search of a lost sequence runs on one lane, latest slot first: frames_pitch is a tick's few frames, not a log.  d_scans_out must
 * not overlap d_scans.  Refused before anything is enqueued, LSD_ERR_INVALID, outputs untouched: a null pointer (d_key may be NULL); n_seq
 * outside 1..65536; frames_pitch outside 1..4096; pose_pitch < 24 or not a multiple of 8; stride outside 1..the context's scan capacity;
 * max_lost outside 1..4096; d_carry or d_poses not 8-byte, d_scans or d_scans_out not 16-byte, d_key, d_lens, d_lens_out, d_pick or
 * d_n_lost not 4-byte aligned. */
int lsd_enqueue_fa_lost_gather_device(lsd_ctx *ctx, const lsd_fa_carry *d_carry, int n_seq, int frames_pitch, const void *d_poses,
                                      size_t pose_pitch, const lsd_polar *d_scans, const int *d_lens, int stride, const int32_t *d_key,
                                      int32_t key, int max_lost, lsd_polar *d_scans_out, int *d_lens_out, int32_t *d_pick,
                                      int32_t *d_n_lost /* [2] */, void *stream);
/* lsd_enqueue_fa_carry_seed_device writes located poses into carries that have none, in place on d_carry[0..n_seq), asynchronous on
 * `stream`, one launch, no workspace, no atomics: it allocates nothing and waits for nothing.  d_pick[n_pick] is the gather's, d_loc[n_pick]
 * the locate records of the gathered rows, d_resp[n_pick] (may be NULL) the response records at those rows.  fp64 without FMA.  Per j the
 * first test that fires decides; each outcome is exactly one flag; the carry keeps every byte unless the outcome is SEEDED.  Report: pose
 * and ang_diff are +0.0 unless SEEDED; seq and slot are -1 for UNUSED, else d_pick[j] / frames_pitch and d_pick[j] % frames_pitch;
 * loc_flags is d_loc[j].flags from step 3 on, 0 before:
 *   0. d_pick[j] < 0: UNUSED
 *   1. s = d_pick[j] / frames_pitch >= n_seq: BAD_PICK; nothing is touched
 *   2. the carry's x[0] no longer passes fabs(x[0] + 1) < 0.0001: HAS_POSE -- the robot found itself, or was seeded, since the gather
 *   3. d_loc[j].flags != LSD_GRID_LOCATE_ACCEPTED: NOT_LOCATED
 *   4. d_loc[j].n_best > par.max_best: AMBIGUOUS (several candidates tie the winner: the map does not tell them apart)
 *   5. with d_resp: VALID clear, or NONE, EMPTY or MISMATCH set: NO_RESPONSE; x, y, ang or one of cov[0..5] not finite: NOT_FINITE (the
 *      correction's step 4).  Without d_resp: the located x, y or ang not finite: NOT_FINITE
 *   6. SEEDED.  z = the located (x, y, ang); with d_resp the response's.  state.x = (z[0], z[1], z[2], +0.0 x 6).  state.P = +0.0 but for
 *      the entries 3..8 of the diagonal, (1, 1, 1, .1, .1, .1) as lsd_fa_initial_state has them, and the leading block: without d_resp the
 *      diagonal (var_xy, var_xy, var_ang); with d_resp R of the correction's step 5 from cov_scale, floor_xy and floor_ang, written
 *      symmetric.  The loop's bookkeeping is its own lines (k_fa.hip; the reference's main_on_windows.cpp:165-172) applied as to a first
 *      frame, REPLACING what the carry held:  d = z[2] - atand(carry.odom.ang);  off = fabs(d) > 90;  if (off && d < 0) d += 360;
 *      ang_sum = 0.0 + d;  ang_count = 1.0;  is_offset = off.  odom and frames keep their bytes, so the cnt_frame == 1 test of the next
 *      frame stays the sequence's own, and its theta is d / 1 where a hand-made carry with no offsets gives 0 / 0 (see
 *      lsd_enqueue_localize_device).  Replaced and not appended: the reset frames in front have each pushed 0 - atand(odom) into the mean,
 *      which is no offset between the map and the odometry at all
 * Two j never name one sequence when d_pick is the gather's; a hand-made d_pick that names a sequence twice is the caller's error (the
 * two writes race).  d_rep may be NULL.  Refused before anything is enqueued, LSD_ERR_INVALID, outputs untouched: a null ctx, d_carry,
 * d_pick or d_loc; n_seq <= 0; frames_pitch outside 1..4096; n_pick outside 1..4096; max_best == 0; one of the five real parameters not
 * finite or negative; var_xy or var_ang not > 0 where d_resp is NULL; d_carry, d_loc, d_resp or d_rep not 8-byte, d_pick not 4-byte
 * aligned. */
typedef struct lsd_grid_locate_rec lsd_grid_locate_rec;
typedef struct lsd_fa_seed_par { double var_xy, var_ang, cov_scale, floor_xy, floor_ang; uint32_t max_best, reserved; } lsd_fa_seed_par;   /* 48 bytes */
typedef struct lsd_fa_seed_rep {                                                                                                          /* 48 bytes */
    double pose[3]; double ang_diff; int32_t seq, slot; uint32_t flags, loc_flags;
} lsd_fa_seed_rep;
enum { LSD_FA_SEED_SEEDED = 1, LSD_FA_SEED_UNUSED = 2, LSD_FA_SEED_BAD_PICK = 4, LSD_FA_SEED_HAS_POSE = 8, LSD_FA_SEED_NOT_LOCATED = 16,
       LSD_FA_SEED_AMBIGUOUS = 32, LSD_FA_SEED_NO_RESPONSE = 64, LSD_FA_SEED_NOT_FINITE = 128 };
int lsd_enqueue_fa_carry_seed_device(lsd_ctx *ctx, lsd_fa_carry *d_carry, int n_seq, int frames_pitch, const int32_t *d_pick, int n_pick,
                                     const lsd_grid_locate_rec *d_loc, const lsd_grid_response_rec *d_resp /* may be NULL */,
                                     lsd_fa_seed_par par, lsd_fa_seed_rep *d_rep /* may be NULL */, void *stream);
/* Host conveniences: the arrays are host arrays of any alignment (the rules above are about device memory, which the context's staging
 * supplies), every sequence takes part (no key).  Blocking.
 * lsd_fa_lost_gather: carries (n_seq), poses (n_seq x frames_pitch, packed), scans (n_seq x frames_pitch x stride) and lens (n_seq x
 * frames_pitch) travel to the context's staging with scans_out (max_lost x stride: the rows past the gathered ones come back as they
 * went), the gather runs, scans_out, lens_out, pick and n_lost come back.  lens[i] outside 0..stride: LSD_ERR_INVALID.
 * lsd_fa_carry_seed: carries (n_seq, updated in place), pick, loc, resp (n_pick each; resp may be NULL) and rep (n_pick, may be NULL). */
int lsd_fa_lost_gather(lsd_ctx *ctx, const lsd_fa_carry *carries, int n_seq, int frames_pitch, const lsd_position *poses,
                       const lsd_polar *scans, const int *lens, int stride, int max_lost, lsd_polar *scans_out, int *lens_out,
                       int32_t *pick, int32_t *n_lost /* [2] */);
int lsd_fa_carry_seed(lsd_ctx *ctx, lsd_fa_carry *carries, int n_seq, int frames_pitch, const int32_t *pick, int n_pick,
                      const lsd_grid_locate_rec *loc, const lsd_grid_response_rec *resp, lsd_fa_seed_par par, lsd_fa_seed_rep *rep);
/* Host convenience: replays one whole log.  scans: n_frames lidar frames at a pitch of `stride` readings, frame t holding lens[t]
 * finite readings (the driver drops the infinite ranges, :115-121); odom: n_frames + 1 rows (the Odom vector); init NULL: the
 * initial state (a reset state, see lsd_enqueue_localize_device).  Runs FeatureScan on every frame, then the loop; states / reports:
 * n_frames records.  LSD_ERR_CAPACITY if a scan
 * marks more than 8192 pixels or has more than 360 lines (the records are then computed from the stored part). */
int lsd_localize(lsd_ctx *ctx, const double *map_cache, int cols, int rows, const lsd_line *map_lines, int n_map, const lsd_polar *scans,
                 const int *lens, int n_frames, int stride, const lsd_position *odom, lsd_map_param map_param, const lsd_fa_state *init,
                 lsd_fa_state *states, lsd_fa_report *reports);
/* Test hook: the fusion kernel alone on a caller-given candidate list (n x {x, y, ang, score}, in single-thread order; n may
 * be 0) with lastPose, ScanPose and the state in. */
int lsd_debug_fa_fuse(lsd_ctx *ctx, const lsd_match_score *cands, int n, lsd_position last_pose, lsd_position scan_pose,
                      const lsd_fa_state *in, lsd_fa_state *out, lsd_fa_report *report);

/* --- wire format (SURVEY 8f "next" #3) ---------------------------------------------------------- */
/* Replaces the cell loop of the ROS map callback (LSD/main_on_linux.cpp:108-124): nav_msgs/OccupancyGrid cells
 * (int8: -1 unknown, 0 free, 1..100 occupied) become the loader's map values (0 unknown, 255 free, 1 occupied), the
 * input of lsd_map_cache and lsd_run.  Host buffers: grid rows x cols packed, map_out with pitch map_stride. */
int lsd_occupancy_to_map(lsd_ctx *ctx, const int8_t *grid, int cols, int rows, uint8_t *map_out, size_t map_stride);
/* The same for n_cells device-resident cells (any number of equally sized grids back to back), asynchronous on
 * `stream`; both pointers 16-byte aligned.  Lets a map that arrives on the device never touch the host. */
int lsd_enqueue_occupancy_to_map_device(lsd_ctx *ctx, const int8_t *d_grid, size_t n_cells, uint8_t *d_map, void *stream);

/* --- the map callback as one enqueue ------------------------------------------------------------ */
/* Replaces the body of mapCallback (LSD/main_on_linux.cpp:97-134) for a grid that is already on the device, asynchronous on `stream`,
 * in the callback's order:
 *   1. the cells of d_grid (rows x cols int8, packed) -> d_map (rows x cols uint8), as lsd_enqueue_occupancy_to_map_device (:108-124);
 *   2. createMapCache(d_map, res, z_occ_max_dis) -> d_map_cache (rows x cols doubles), read BEFORE the detector rewrites the map (:130;
 *      the callback passes z_occ_max_dis = 2, :126-127);
 *   3. myLineSegmentDetector on d_map with LSD_FLAG_WRITEBACK_MAP (:132): d_map ends as the callback's mapValue does, d_lines (max_lines
 *      records) and *d_count are structLSD.linesInfo / len_linesInfo, d_line_im (rows x cols uint8, or NULL) is structLSD.lineIm.
 * *d_count follows lsd_enqueue_batch_device: above max_lines the map overflowed (its first max_lines records are valid), -1 the region
 * stage gave the map up.  Argument errors -- a null pointer other than d_line_im, a non-positive size, d_grid or d_map not 16-byte
 * aligned (LSD_ERR_INVALID), cols * rows >= 2^31 or parameters the detector refuses (LSD_ERR_UNSUPPORTED) -- are found before anything
 * is enqueued.  Like every enqueue that uses the context's workspace, an update on another stream than the context's last detector run
 * is ordered behind that run by an event (never a host wait); apart from that one context serves one stream at a time, so a caller
 * that localises on one stream while maps are made on another gives the map side a context of its own (Localizer does). */
int lsd_enqueue_map_update_device(lsd_ctx *ctx, const int8_t *d_grid, int cols, int rows, double res, double z_occ_max_dis,
                                  const lsd_params *p, uint8_t *d_map, double *d_map_cache, lsd_line *d_lines, int max_lines,
                                  int32_t *d_count, uint8_t *d_line_im, void *stream);
/* Sizes what lsd_enqueue_map_update_device allocates for a cols x rows grid: lsd_reserve(ctx, 1, cols, rows) with the detector's record
 * arrays for up to the host line capacity (lsd_set_host_max_lines, default 8192) per map, createMapCache's scratch, and the lookup
 * tables of the default parameters.  After it an update of that size or smaller, with the default parameters and max_lines up to that
 * capacity, makes no allocation, no blocking copy and no host wait. */
int lsd_reserve_map_update(lsd_ctx *ctx, int cols, int rows);

/* --- mapping with known poses: localised scans into an OccupancyGrid ------------------------------ */
/* No reference counterpart: the reference's maps come from an outside SLAM (Karto) that re-publishes the grid.  These entries turn the
 * scans and poses a fleet has on the device every tick into that grid.  These entries take a pose as it is; the section after this one corrects
 * it against the growing grid first (correlative scan-to-grid matching).  No loop closure.  The map state is two caller-owned device planes of rows x cols uint32, d_pass and d_hit (Karto's counting model), in the
 * frame map_param names; the entries ADD to them (clear them with hipMemsetAsync).  Counters wrap at 2^32.
 * lsd_enqueue_grid_integrate_device: n_scans scans as the ingest entries write them (d_scans at a pitch of `stride` readings, d_lens),
 * scan i at the pose (x, y in map pixels, ang in degrees: the rotation of the scan frame onto the map) held in the first three doubles of
 * the record at d_poses + i * pose_pitch_bytes -- packed lsd_position (24), an array of lsd_fa_state (720) or of lsd_fa_carry (768) as
 * it is.  One launch, asynchronous on `stream`, no workspace, no synchronisation.  The rule, fp64 without FMA:
 *   scan skipped whole   a pose component not finite; |x + 1| < 1e-4 (the reference's "no pose" test, LSD/myFA.cpp:99); |x| or |y| > 2^20
 *   beam i < len skipped range NaN, <= 0 or +inf; angle not finite; angle + ang / 180 * pi not finite
 *   rr = min(range, range_max); the beam HITS iff range <= range_max;  th = angle + ang / 180.0 * pi;  (s, c) = sin, cos(th), correctly
 *   rounded;  x0 = (int)round(x), y0 = (int)round(y), x1 = (int)round(x + rr * c / mapResol), y1 = (int)round(y + rr * s / mapResol)
 *   the ray: dx = x1 - x0, dy = y1 - y0, n = max(|dx|, |dy|), m = min(|dx|, |dy|), the major axis x iff |dx| >= |dy|; for k = 0 .. n the
 *   cell with major = start + k * sgn, minor = start + sgn_minor * ((2 k m + n) / (2 n)) in integers; n = 0: the start cell alone
 *   every cell of the ray inside [0, cols) x [0, rows) gets pass += 1; a beam that hits and whose cell k = n is inside gives it hit += 1
 * Refused before anything is enqueued, LSD_ERR_INVALID: a null pointer, n_scans < 0, stride <= 0 or above the context's scan capacity,
 * cols or rows outside 1..65535, mapResol or range_max not > 0, range_max / mapResol >= 32767 (keeps 2 k m + n within 32 bits), a pitch
 * below 24 or not a multiple of 8, d_scans not 16-byte or d_poses not 8-byte aligned.  n_scans == 0 launches nothing. */
int lsd_enqueue_grid_integrate_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                      const void *d_poses, size_t pose_pitch_bytes, lsd_map_param map_param, double range_max,
                                      uint32_t *d_pass, uint32_t *d_hit, void *stream);
/* The planes as the int8 row-major grid lsd_enqueue_map_update_device and lsd_enqueue_occupancy_to_map_device take, integers only:
 *   d_grid[i] = -1 if d_pass[i] < min_pass, else 100 if (uint64) d_hit[i] * occ_den >= (uint64) d_pass[i] * occ_num, else 0.
 * Karto's min_pass_through and occupancy_threshold are min_pass = 2, occ_num / occ_den = 1 / 10.  LSD_ERR_INVALID for a null pointer,
 * n_cells == 0, occ_den == 0 or occ_num > occ_den.  One launch, asynchronous on `stream`. */
int lsd_enqueue_grid_publish_device(lsd_ctx *ctx, const uint32_t *d_pass, const uint32_t *d_hit, size_t n_cells, uint32_t min_pass,
                                    uint32_t occ_num, uint32_t occ_den, int8_t *d_grid, void *stream);
/* Host convenience: scans, lens, poses (n_scans packed lsd_position) and the two planes (rows x cols of map_param, IN-OUT) travel to the
 * context's staging, lsd_enqueue_grid_integrate_device runs, the planes come back.  Blocking.  lens[i] outside 0..stride:
 * LSD_ERR_INVALID. */
int lsd_grid_integrate(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, const lsd_position *poses,
                       lsd_map_param map_param, double range_max, uint32_t *pass, uint32_t *hit);

/* --- correlative scan-to-grid matching: a pose corrected against the growing grid before it is integrated ------- */
/* Scan matching against the growing grid now exists (csrc/k_gridmatch.hip): Olson's / Karto's correlative matcher in
 * its plain, single-resolution form.  The planes are turned into a uint8 lookup plane (every occupied cell smeared by a small table), and
 * each scan's rounded end cells are translated over a window of whole cells and whole angle steps around its pose and summed on that
 * plane.  The result is made of integers and has no iteration order: tests/grid_match_cases.py restates both rules and the device gives
 * the same bytes.  The same match as a coarse-to-fine search: the section after this one; a sub-cell pose and a covariance of the
 * response: the one after that; the search WITHOUT a prior, over the whole grid and all headings: the section on global localisation
 * below.  NOT built: loop closure, the fleet classes.
 * lsd_enqueue_grid_likelihood_device: a cell is OCCUPIED iff the publish rule gives it 100 (d_pass >= min_pass and (uint64) d_hit *
 * occ_den >= (uint64) d_pass * occ_num);  d_corr[y][x] = the maximum of smear.w[|v|][|u|] over all |u|, |v| <= smear.radius for which
 * (x + u, y + v) is inside the grid and occupied, 0 if there is none (a maximum has no order: the table need not be monotone).  One
 * launch, no workspace, asynchronous.  LSD_ERR_INVALID before anything is enqueued: a null pointer, cols or rows outside 1..65535, a
 * radius outside 0..7, occ_den == 0 or occ_num > occ_den.
 * lsd_grid_smear_default (host only, a convenience): w[|v|][|u|] = (uint8) floor(255 * exp(-(u^2 + v^2) / (2 sigma_cells^2)) + 0.5) for
 * |u|, |v| <= radius with the host's libm, 0 elsewhere.  LSD_ERR_INVALID: out null, radius outside 0..7, sigma_cells not finite or <= 0. */
typedef struct lsd_grid_smear { int radius; uint8_t w[8][8]; } lsd_grid_smear;   /* radius 0..7, w[|dv|][|du|] */
int lsd_enqueue_grid_likelihood_device(lsd_ctx *ctx, const uint32_t *d_pass, const uint32_t *d_hit, int cols, int rows,
                                       uint32_t min_pass, uint32_t occ_num, uint32_t occ_den, lsd_grid_smear smear, uint8_t *d_corr,
                                       void *stream);
int lsd_grid_smear_default(double sigma_cells, int radius, lsd_grid_smear *out);
/* lsd_enqueue_grid_match_device: scans, lengths and poses as lsd_enqueue_grid_integrate_device reads them, d_corr a rows x cols plane of
 * map_param's grid.  Everything is fp64 without FMA, with the integration's own helpers.  For scan n at pose (x, y, ang):
 *   skipped scans and beams   the integration's tests (above); a skipped scan's record: its pose's 24 bytes, flags = 2, every other field 0
 *   candidates  (a, j, i), a in -na..na, j in -wy..wy, i in -wx..wx;  theta_a = ang + (double) a * ang_step (a multiply, then an add)
 *   a beam is SCORED at angle a iff it is not skipped, range <= range_max and th = angle + theta_a / 180 * pi is finite; its end cell is
 *   ex = (int)round(x + range * cos(th) / mapResol), ey = (int)round(y + range * sin(th) / mapResol); nb(a) counts the scored beams
 *   S(a, j, i) = the sum over the beams scored at a of d_corr[ey + j][ex + i], 0 where that cell is outside the grid (uint32: at most
 *   255 * 4096 < 2^20)
 *   the winner: the largest S, then the smallest i^2 + j^2, then the smallest |a|, then the smallest linear index
 *   ((a + na) * (2 wy + 1) + (j + wy)) * (2 wx + 1) + (i + wx) -- on a featureless plane the prior pose wins
 *   record: score = S of the winner, n_beams = nb of its angle, di, dj, da its offsets, score_prior = S(0, 0, 0), reserved = 0
 *   ACCEPTED (flags bit 0) iff n_beams >= min_beams and (uint64) score * min_den >= (uint64) 255 * n_beams * min_num; then
 *   (x, y, ang) = (x + di, y + dj, theta_da); else the input pose's bits are copied
 * An array of records IS a d_poses argument of pitch 56 for lsd_enqueue_grid_integrate_device.  Two launches, asynchronous on `stream`;
 * the n_scans * (2 na + 1) slots between them (16 bytes each) are context workspace, grown before the first launch when needed -- that
 * case alone synchronises; there is no other allocation, copy or host wait.  LSD_ERR_INVALID before anything is enqueued: whatever
 * lsd_enqueue_grid_integrate_device refuses on the arguments the two share; wx, wy or na outside 0..63; ang_step not finite or negative;
 * ang_step == 0 with na > 0; min_den == 0 or min_num > min_den; d_corr or d_out null, d_out not 8-byte aligned.  n_scans == 0 launches
 * nothing.
 * (The record's type is lsd_grid_match_rec: in C a typedef and the host entry below cannot share the name lsd_grid_match; the struct
 * tag can.) */
typedef struct lsd_grid_search { int wx, wy, na; double ang_step; uint32_t min_beams, min_num, min_den; } lsd_grid_search;
typedef struct lsd_grid_match {            /* 56 bytes; its head is a pose, so an array of these IS a d_poses argument (pitch 56) */
    double x, y, ang; uint32_t score, n_beams; int32_t di, dj, da; uint32_t flags, score_prior, reserved;
} lsd_grid_match_rec;
#define LSD_GRID_MATCH_ACCEPTED 1u
#define LSD_GRID_MATCH_SKIPPED 2u
int lsd_enqueue_grid_match_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                  const void *d_poses, size_t pose_pitch_bytes, lsd_map_param map_param, double range_max,
                                  const uint8_t *d_corr, lsd_grid_search search, lsd_grid_match_rec *d_out, void *stream);
/* Host convenience: scans, lens, poses (n_scans packed lsd_position) and the plane (rows x cols of map_param) travel to the context's
 * staging, lsd_enqueue_grid_match_device runs, the n_scans records come back.  Blocking.  lens[i] outside 0..stride: LSD_ERR_INVALID. */
int lsd_grid_match(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, const lsd_position *poses,
                   lsd_map_param map_param, double range_max, const uint8_t *corr, lsd_grid_search search, lsd_grid_match_rec *out);

/* --- the same match, coarse to fine: a plane of block maxima prunes the window, the records stay the plain entry's byte for byte ---- */
/* Olson's multi-resolution form in two levels (csrc/k_gridmatch_mr.hip; restated in tests/grid_match_mr_cases.py).  The
 * angle axis is not coarsened.  For a block size b = `block` in 2..16:
 *   the coarse plane: (rows + b - 1) x (cols + b - 1) bytes, coarse[y + b - 1][x + b - 1] = the maximum of d_corr[y + v][x + u] over
 *   0 <= u, v < b with (x + u, y + v) inside the grid, 0 if there is none, for x = -(b - 1) .. cols - 1 and y likewise: a sliding maximum
 *   anchored at the block's low corner, at full resolution (the block grid of a search is anchored at -wx, not at the plane)
 *   blocks: nbx = ceil((2 wx + 1) / b), nby likewise; block (a, J, I) covers i = -wx + I b .. min(wx, -wx + I b + b - 1), j likewise
 *   U(a, J, I) = the sum over the beams scored at a of coarse[ey - wy + J b + b - 1][ex - wx + I b + b - 1], 0 where that index is outside
 *   the coarse plane: S <= U for every candidate of the block
 *   the seed of angle a: the block with the largest U(a, ., .), among equals the smallest J nbx + I; L_a = the largest S among the seed's
 *   candidates inside the window; L = the maximum of L_a over the angles
 *   every block with U >= L is REFINED: its candidates inside the window are scored and enter the plain entry's key maximum.  The plain
 *   winner's block has U >= S_win >= L, so it is among them: all 56 bytes of the record are lsd_enqueue_grid_match_device's
 *   score_prior = S(0, 0, 0) and nb(a) are computed whatever is pruned
 *   statistics (d_stats, may be NULL; 16 bytes per scan): blocks = (2 na + 1) nbx nby; refined = the blocks with U >= L; fine = the
 *   candidates inside the window in refined blocks (the seeds' own evaluation is not counted); lower_bound = L; a skipped scan: all 0
 * lsd_enqueue_grid_coarse_device: one launch, no workspace, asynchronous.  LSD_ERR_INVALID before anything is enqueued: a null pointer,
 * cols or rows outside 1..65535, block outside 2..16.  lsd_grid_coarse_bytes: the plane's size, 0 for arguments the entry refuses.
 * lsd_enqueue_grid_match_mr_device: d_coarse is what lsd_enqueue_grid_coarse_device made of d_corr with the same `block`.  Three launches
 * (four with d_stats), asynchronous on `stream`; U (4 bytes per block and angle) and 40 bytes per (scan, angle) are context workspace,
 * grown before the first launch when needed -- that case alone synchronises; there is no other allocation, copy or host wait.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: whatever lsd_enqueue_grid_match_device refuses, block outside 2..16,
 * d_coarse null, d_stats not 4-byte aligned.  n_scans == 0 launches nothing. */
typedef struct lsd_grid_match_mr_stats { uint32_t blocks, refined, fine, lower_bound; } lsd_grid_match_mr_stats;
size_t lsd_grid_coarse_bytes(int cols, int rows, int block);
int lsd_enqueue_grid_coarse_device(lsd_ctx *ctx, const uint8_t *d_corr, int cols, int rows, int block, uint8_t *d_coarse, void *stream);
int lsd_enqueue_grid_match_mr_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                     const void *d_poses, size_t pose_pitch_bytes, lsd_map_param map_param, double range_max,
                                     const uint8_t *d_corr, const uint8_t *d_coarse, int block, lsd_grid_search search,
                                     lsd_grid_match_rec *d_out, lsd_grid_match_mr_stats *d_stats, void *stream);
/* Host convenience: as lsd_grid_match; the coarse plane is built in the context's staging, `stats` (n_scans records) may be NULL.
 * Blocking. */
int lsd_grid_match_mr(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, const lsd_position *poses,
                      lsd_map_param map_param, double range_max, const uint8_t *corr, int block, lsd_grid_search search,
                      lsd_grid_match_rec *out, lsd_grid_match_mr_stats *stats);

/* --- the response around a match: a covariance and a sub-cell, sub-step pose from the scores next to the winner ---------------- */
/* A stage behind either match entry (csrc/k_gridresponse.hip; restated in tests/grid_response_cases.py): it reads the
 * records a match wrote and writes one response record per scan.  Integer sums until one fp64 division per output; fp64 without FMA.
 * Inputs per scan: the scan and its length, its ORIGINAL pose (x, y, ang) -- the one the match was given, at d_poses + n *
 * pose_pitch_bytes --, its lsd_grid_match_rec, the lookup plane, mapResol, range_max and the search's ang_step.
 *   a scan GETS A RESPONSE iff its record has LSD_GRID_MATCH_ACCEPTED set, LSD_GRID_MATCH_SKIPPED clear and |di|, |dj|, |da| <= 63 (the
 *   record is caller memory: the range test makes noise harmless).  Otherwise the response record is the match record's 24 pose bytes,
 *   flags = LSD_GRID_RESPONSE_NONE, every other byte 0, and nothing is scored
 *   candidates  (a', j', i'), a' in -ra..ra, j' in -ry..ry, i' in -rx..rx, centred on the winner;  theta = ang + (double)(da + a') *
 *   ang_step (the match's own expression: at a' = 0 the end cells are the winner's).  The scored beams and their end cells (ex, ey) are
 *   the match's, from the ORIGINAL pose (round(x + di + ..) is not round(x + ..) + di); an original pose the match's scan test skips
 *   (noise again) scores no beam
 *   R(a', j', i') = the sum over the beams scored at theta of d_corr[ey + dj + j'][ex + di + i'], 0 outside the grid.  The window may
 *   leave the search's.  score_centre = R(0, 0, 0); it equals the record's score for an authentic record, else
 *   LSD_GRID_RESPONSE_MISMATCH is set and the record's score is used as given
 *   a candidate is USED iff (uint64) R * keep_den >= (uint64) score * keep_num; its weight w is then R, else 0.  n_used counts them.
 *   m[10] (int64, each < 2^38: exact, no order) = sum w, sum w i', w j', w a', w i'^2, w i'j', w j'^2, w i'a', w j'a', w a'^2
 *   covariance about the winner (Karto's), with W = m[0] > 0:  cov = { (double) m[4] / (double) W, m[5] / W, m[6] / W  (pixels^2),
 *   (m[7] / W) * ang_step, (m[8] / W) * ang_step, (m[9] / W) * (ang_step * ang_step) };  W == 0: six zeros and LSD_GRID_RESPONSE_EMPTY
 *   sub-cell offsets, per axis: m_ and p_ the R one step below and above the centre (the other two offsets 0), c = score_centre, num =
 *   m_ - p_, den = 2 (m_ - 2 c + p_) in int64.  m_ > c, p_ > c or den >= 0: +0.0 and the axis's NOT_PEAK bit (a plateau, or a winner on
 *   the rim of the search window with a higher neighbour outside).  Else num == 0: +0.0 (0 / den would be -0.0).  Else (double) num /
 *   (double) den, within +-0.5.  ra == 0: the angle offset is +0.0 with no flag.  sub = { x, y, a } offsets
 *   the refined pose: x = rec.x + sub[0], y = rec.y + sub[1], ang = rec.ang + sub[2] * ang_step
 * The record's head is a pose: an array of them IS a d_poses argument of pitch 192 for lsd_enqueue_grid_integrate_device.
 * d_volume may be NULL; otherwise it receives n_scans x (2 ra + 1)(2 ry + 1)(2 rx + 1) uint32 values of R, i' fastest, zeros for a scan
 * without a response (lsd_grid_response_volume_bytes: its size; 0 for arguments the entry refuses).  With NULL the volume is context
 * workspace, grown before the first launch when needed -- that case alone synchronises; there is no other allocation, copy or host wait.
 * Two launches, asynchronous on `stream`.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: whatever
 * lsd_enqueue_grid_match_device refuses on the arguments the two share; rx or ry outside 1..7, ra outside 0..7; keep_den == 0 or
 * keep_num > keep_den; ang_step not finite or negative, ang_step == 0 with ra > 0; d_records or d_out null or not 8-byte aligned;
 * d_volume not 4-byte aligned.  n_scans == 0 launches nothing.
 * (The parameters' type is lsd_grid_response_par: the host entry below has the struct tag's name.) */
typedef struct lsd_grid_response { int rx, ry, ra; uint32_t keep_num, keep_den; } lsd_grid_response_par;
typedef struct lsd_grid_response_rec {     /* 192 bytes; its head is a pose, so an array of these IS a d_poses argument (pitch 192) */
    double x, y, ang;
    double cov[6];                         /* xx, xy, yy, xa, ya, aa */
    double sub[3];                         /* x, y, a */
    int64_t m[10];
    uint32_t score_centre, n_used, flags, reserved;
} lsd_grid_response_rec;
#define LSD_GRID_RESPONSE_VALID 1u
#define LSD_GRID_RESPONSE_NONE 2u
#define LSD_GRID_RESPONSE_X_NOT_PEAK 4u
#define LSD_GRID_RESPONSE_Y_NOT_PEAK 8u
#define LSD_GRID_RESPONSE_A_NOT_PEAK 16u
#define LSD_GRID_RESPONSE_EMPTY 32u
#define LSD_GRID_RESPONSE_MISMATCH 64u
size_t lsd_grid_response_volume_bytes(int n_scans, lsd_grid_response_par response);
int lsd_enqueue_grid_response_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                     const void *d_poses, size_t pose_pitch_bytes, const lsd_grid_match_rec *d_records,
                                     lsd_map_param map_param, double range_max, const uint8_t *d_corr, double ang_step,
                                     lsd_grid_response_par response, lsd_grid_response_rec *d_out, uint32_t *d_volume, void *stream);
/* Host convenience: as lsd_grid_match, with the n_scans match records; `volume` (lsd_grid_response_volume_bytes bytes) may be NULL.
 * Blocking. */
int lsd_grid_response(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, const lsd_position *poses,
                      const lsd_grid_match_rec *records, lsd_map_param map_param, double range_max, const uint8_t *corr,
                      double ang_step, lsd_grid_response_par response, lsd_grid_response_rec *out, uint32_t *volume);

/* --- ray casting on the grid: the expected range of every beam, its class against the map, a screened scan ---------------------- */
/* What a scan should look like from a pose (csrc/k_gridray.hip; restated in tests/grid_ray_cases.py).  Scans, lengths
 * and poses as lsd_enqueue_grid_integrate_device reads them; d_grid is an int8 rows x cols OccupancyGrid of map_param's frame, the layout
 * lsd_enqueue_grid_publish_device writes and lsd_enqueue_map_update_device reads (an outside SLAM's map serves as well).  A cell is read
 * as the map update reads it: byte 255 unknown, 0 free, every other byte occupied; a cell outside the grid is unknown.  fp64 without FMA,
 * the integration's helpers.  For scan n at pose (x, y, ang):
 *   a scan the integration skips whole is not cast; beam i < len is CAST iff its angle and th = angle + ang / 180.0 * pi are finite (the
 *   measured range plays no part);  (s, c) = sin, cos(th);  x0 = (int)round(x), y0 = (int)round(y), x1 = (int)round(x + range_max * c /
 *   mapResol), y1 = (int)round(y + range_max * s / mapResol);  the ray's cells k = 0 .. n: the integration's closed form, start cell included
 *   k_hit = the smallest k whose cell is occupied, else -1;  k_unk = the smallest k whose cell is unknown and that lies before k_hit (any k
 *   if there is no hit), else -1
 *   dist(k) = sqrt(ddx * ddx + ddy * ddy) * mapResol with ddx = (double) cx_k - x, ddy = (double) cy_k - y;  r_exp = dist(k_hit) or +inf,
 *   r_unk = dist(k_unk) or +inf;  (cx, cy) = the hit cell, or (x1, y1) without one
 *   the class, with m the measured range and d = m - r_exp:  not cast: NOT_CAST, every other byte of the record 0;  m NaN or <= 0:
 *   NO_MEASUREMENT;  m == +inf or m > range_max: LONG with a hit, else UNEXPLORED with an unknown cell, else AGREE_FREE;  otherwise
 *   |d| <= tol: AGREE;  d > tol: LONG;  else r_unk <= m: UNEXPLORED;  else SHORT (something in front of what the map holds)
 * The ray runs to the range_max end cell, not to the measured one, so it can pass one cell beside the cell in which the integration
 * counted the beam's hit; tol absorbs that.
 * d_out: the record of beam i of scan n at d_out[n * stride + i], i < len only (slots beyond stay untouched).  d_sum[n]: the input pose's
 * bits, n[c] = the beams of class c over i < len, judged = n[2] + n[3] + n[4] + n[5]; CONSISTENT iff judged >= min_beams and (uint64)
 * (n[2] + n[3]) * ok_den >= (uint64) judged * ok_num; a scan skipped whole: SKIPPED, all counts 0.  With gate != 0 a scan that was cast
 * and is not consistent gets x = -1.0 (the "no pose" sentinel; y and ang stay): an array of these records IS a d_poses argument of pitch
 * 64, and every grid entry then skips that scan by the rule it has.
 * d_scans_out (may be NULL; rows at the pitch of d_scans): for i < len the angle's bits, and the range's bits unless (drop_mask >> class)
 * & 1, then the quiet NaN 0x7FF8000000000000, which integration, both matchers and the response skip.  d_scans_out == d_scans is
 * allowed (a beam is read and written by the same lane); any other overlap of the two is refused.
 * Two launches, asynchronous on `stream`; no workspace, no allocation, copy or host wait.  LSD_ERR_INVALID before anything is enqueued,
 * outputs untouched: whatever lsd_enqueue_grid_integrate_device refuses on the arguments the two share; d_grid, d_out or d_sum null; tol
 * not finite or negative; drop_mask >= 128; ok_den == 0 or ok_num > ok_den; d_out or d_sum not 8-byte aligned; d_scans_out not 16-byte
 * aligned or partially overlapping d_scans.  n_scans == 0 launches nothing.
 * (The parameters' type is lsd_grid_ray_par and the record's lsd_grid_ray; the host entry is lsd_grid_raycast.) */
typedef struct lsd_grid_ray_par { double tol; uint32_t drop_mask, min_beams, ok_num, ok_den; int gate; } lsd_grid_ray_par;
typedef struct lsd_grid_ray {              /* 32 bytes */
    double r_exp, r_unk; int32_t cx, cy, k_hit; uint32_t cls;
} lsd_grid_ray;
typedef struct lsd_grid_ray_sum {          /* 64 bytes; its head is a pose, so an array of these IS a d_poses argument (pitch 64) */
    double x, y, ang; uint32_t n[7]; uint32_t judged; uint32_t flags; uint32_t pad;
} lsd_grid_ray_sum;
#define LSD_GRID_RAY_NOT_CAST 0u
#define LSD_GRID_RAY_NO_MEASUREMENT 1u
#define LSD_GRID_RAY_AGREE_FREE 2u
#define LSD_GRID_RAY_AGREE 3u
#define LSD_GRID_RAY_SHORT 4u
#define LSD_GRID_RAY_LONG 5u
#define LSD_GRID_RAY_UNEXPLORED 6u
#define LSD_GRID_RAY_CONSISTENT 1u
#define LSD_GRID_RAY_SKIPPED 2u
int lsd_enqueue_grid_raycast_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                    const void *d_poses, size_t pose_pitch_bytes, lsd_map_param map_param, double range_max,
                                    const int8_t *d_grid, lsd_grid_ray_par par, lsd_grid_ray *d_out, lsd_grid_ray_sum *d_sum,
                                    lsd_polar *d_scans_out, void *stream);
/* Host convenience: scans, lens, poses (n_scans packed lsd_position) and the grid (rows x cols of map_param) travel to the context's
 * staging, lsd_enqueue_grid_raycast_device runs, and `out` (n_scans * stride records; those at i < len are written), `sum` (n_scans
 * records) and, unless NULL, `scans_out` (n_scans * stride readings; those at i < len are written) come back.  Blocking.  lens[i]
 * outside 0..stride: LSD_ERR_INVALID. */
int lsd_grid_raycast(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, const lsd_position *poses,
                     lsd_map_param map_param, double range_max, const int8_t *grid, lsd_grid_ray_par par, lsd_grid_ray *out,
                     lsd_grid_ray_sum *sum, lsd_polar *scans_out);

/* --- global scan-to-grid localisation: the match without a prior, exact branch and bound over a pyramid of block maxima --------- */
/* Every entry above searches at most +-63 cells and steps around a pose that is nearly right.  This one has no prior: it searches a whole
 * box of lidar cells and a whole fan of headings on the lookup plane (csrc/k_gridlocate.hip; restated in
 * tests/grid_locate_cases.py).  Branch and bound over a max-pyramid (Olson; Cartographer's fast correlative matcher), held to the
 * exhaustive search byte for byte: the winner's order is made of integers.  fp64 without FMA, the integration's helpers.  The heading
 * axis is not coarsened.  Writing the located pose into a reset carry is lsd_enqueue_fa_lost_gather_device / lsd_enqueue_fa_carry_seed_device
 * above (the section "relocalisation on the device"), around this entry as it is.  NOT built: loop closure proper.
 *   candidates  (a, q, p), a < n_ang, q < ny, p < nx: the lidar at cell (x0 + p, y0 + q), the heading theta_a = ang0 + (double) a *
 *   ang_step;  lin = ((uint64) a * ny + q) * nx + p.  The box may overhang or leave the grid
 *   a beam is SCORED at a iff the integration does not skip it at the pose (0, 0, theta_a), range <= range_max and th = angle + theta_a /
 *   180 * pi is finite; its offset is ox = (int)round(range * cos(th) / mapResol), oy likewise with sin -- the match's end cell at the
 *   pose (0, 0, theta_a), NOT round(cx + d) -- once per (beam, heading); nb(a) counts the scored beams
 *   S(a, q, p) = the sum over the beams scored at a of corr[y0 + q + oy][x0 + p + ox], 0 outside the grid
 *   the winner: the largest S, then the smallest lin;  n_best = the candidates whose S is the winner's (the ambiguity a caller must see
 *   before trusting a relocalisation)
 *   the pyramid: plane_0 = corr; for h = 1..levels plane_h is (rows + 2^h - 1) x (cols + 2^h - 1) bytes, plane_h[y + 2^h - 1][x + 2^h - 1]
 *   = the maximum of corr over [x, x + 2^h) x [y, y + 2^h) inside the grid, 0 if none (the coarse plane of the section above at b = 2^h),
 *   built level from level: four reads of plane_(h-1) at stride 2^(h-1).  The planes 0..levels lie one behind the other in one caller-owned
 *   buffer: lsd_grid_pyramid_bytes its size (0 for arguments the entry refuses), lsd_grid_pyramid_offset(cols, rows, h) where level h
 *   starts ((size_t)-1 for arguments the entry refuses).  A buffer built with more levels serves a search with fewer
 *   nodes: node (a, Q, P) of level h covers p in [P 2^h, min(nx, (P + 1) 2^h)) and q likewise; a node whose low corner is outside the box
 *   does not exist.  U_h = the sum over the beams scored at a of plane_h at the cell (x0 + P 2^h + ox, y0 + Q 2^h + oy), 0 outside the
 *   plane.  Beam by beam a node bounds its children: U_H >= .. >= U_1 >= U_0 = S
 *   the lower bound: per heading start at the top node (h = H = levels) with the largest U_H, among equals the smallest Q nbx + P (nbx =
 *   ceil(nx / 2^H)); descend to the existing child with the largest U, among equals the smallest (Q, P) in that order, down to a candidate;
 *   L_a = its S;  L = max(max_a L_a, score_floor)
 *   the frontier: F_H = the top nodes with U_H >= L; F_(h-1) = the existing children of F_h with U >= L; F_0 = the candidates reached with
 *   S >= L.  Every candidate that ties the winner is in F_0 when score_floor <= S_win, so the maximum over F_0 and the count of its
 *   equals are the exhaustive search's.  levels = 0: the top nodes are the candidates themselves
 *   the outcome, exactly one of the flags:  EMPTY nb(a) == 0 for every heading, nothing is searched;  OVERFLOW some |F_h| > max_nodes, h in
 *   1..H -- the count is exact, the level and those below it are not run (a featureless plane ends here: the right answer for an
 *   ambiguous map);  NOT_FOUND F_0 is empty (only a score_floor above S_win does that);  REJECTED a winner, but n_beams < min_beams or
 *   (uint64) score * min_den < (uint64) 255 * n_beams * min_num;  ACCEPTED otherwise
 *   record: ACCEPTED: (x, y, ang) = ((double) cx, (double) cy, theta_a); every other outcome: the "no pose" sentinel (-1.0, -1.0, +0.0),
 *   which the integration and the match skip.  cx = x0 + p, cy = y0 + q, a, score = S, n_beams = nb(a), n_best: the winner's, for REJECTED
 *   too, 0 without a winner;  lower_bound = L, 0 for EMPTY;  reserved = 0.  An array of records IS a d_poses argument of pitch 64
 *   statistics (d_stats, may be NULL; 48 bytes per scan): top_nodes = n_ang nbx nby;  frontier[h] = |F_h| for h <= H, 0 above H and below
 *   an overflow;  scored = top_nodes + the existing children evaluated;  EMPTY: all 0
 * lsd_enqueue_grid_pyramid_device: levels + 1 launches (level 0 copies d_corr), no workspace, asynchronous.  LSD_ERR_INVALID before
 * anything is enqueued: a null pointer, cols or rows outside 1..65535, levels outside 0..8.
 * lsd_enqueue_grid_locate_device: d_pyramid is what lsd_enqueue_grid_pyramid_device made of the lookup plane with at least par.levels
 * levels.  levels + 5 launches (offsets, top level, bound, frontier seed, one expansion per level, pick), a number fixed by the
 * parameters and never by the data; asynchronous on `stream`.  The workspace (lsd_grid_locate_workspace_bytes: 4 bytes per beam and
 * heading, 4 bytes per top node, 16 bytes per node of max_nodes where levels > 0, and 16 KiB, all per scan; 0 for arguments the entry
 * refuses) is the context's, grown before the first launch when needed -- that case alone synchronises; there is no other allocation,
 * copy or host wait.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: whatever lsd_enqueue_grid_match_device refuses on
 * n_scans, stride, map_param and range_max; x0 or y0 beyond +-2^20; nx or ny outside 1..65535; n_ang outside 1..4096; ang0 or ang_step not
 * finite, ang_step negative, ang_step == 0 with n_ang > 1; levels outside 0..8; max_nodes outside 1..2^24; min_den == 0 or min_num >
 * min_den; more than 2^28 top nodes; d_scans, d_lens, d_pyramid or d_out null; d_scans not 16-byte, d_out not 8-byte, d_stats not 4-byte
 * aligned.  n_scans == 0 launches nothing.
 * (The parameters' type is lsd_grid_locate_par and the record's lsd_grid_locate_rec: the host entry has the name lsd_grid_locate.) */
#define LSD_GRID_LOCATE_MAX_LEVELS 8
typedef struct lsd_grid_locate_par {       /* 64 bytes */
    int x0, y0, nx, ny; double ang0, ang_step; int n_ang, levels; uint32_t max_nodes, score_floor, min_beams, min_num, min_den;
} lsd_grid_locate_par;
typedef struct lsd_grid_locate_rec {       /* 64 bytes; its head is a pose, so an array of these IS a d_poses argument (pitch 64) */
    double x, y, ang; uint32_t score, n_beams; int32_t cx, cy, a; uint32_t flags, n_best, lower_bound, reserved[2];
} lsd_grid_locate_rec;
typedef struct lsd_grid_locate_stats { uint32_t top_nodes, frontier[9], scored, reserved; } lsd_grid_locate_stats;   /* 48 bytes */
#define LSD_GRID_LOCATE_ACCEPTED 1u
#define LSD_GRID_LOCATE_REJECTED 2u
#define LSD_GRID_LOCATE_NOT_FOUND 4u
#define LSD_GRID_LOCATE_OVERFLOW 8u
#define LSD_GRID_LOCATE_EMPTY 16u
size_t lsd_grid_pyramid_bytes(int cols, int rows, int levels);
size_t lsd_grid_pyramid_offset(int cols, int rows, int h);
int lsd_enqueue_grid_pyramid_device(lsd_ctx *ctx, const uint8_t *d_corr, int cols, int rows, int levels, uint8_t *d_pyramid, void *stream);
size_t lsd_grid_locate_workspace_bytes(int n_scans, int stride, lsd_grid_locate_par par);
int lsd_enqueue_grid_locate_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                   lsd_map_param map_param, double range_max, const uint8_t *d_pyramid, lsd_grid_locate_par par,
                                   lsd_grid_locate_rec *d_out, lsd_grid_locate_stats *d_stats, void *stream);
/* Host convenience: scans, lens and the lookup plane (rows x cols of map_param) travel to the context's staging, the pyramid is built
 * there, lsd_enqueue_grid_locate_device runs, the n_scans records and, unless NULL, the n_scans statistics records come back.  Blocking.
 * lens[i] outside 0..stride: LSD_ERR_INVALID. */
int lsd_grid_locate(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, lsd_map_param map_param,
                    double range_max, const uint8_t *corr, lsd_grid_locate_par par, lsd_grid_locate_rec *out,
                    lsd_grid_locate_stats *stats);

/* --- the same search with the bound tightened level by level, and a level that overflows retried once ------------------------------- */
/* The entry above fixes L once, from one greedy descent per heading that starts at the top level, and never raises it.  This one
 * (csrc/k_gridlocate_tight.hip; restated in tests/grid_locate_tight_cases.py) is the same search -- the same candidates,
 * offsets, S, pyramid, nodes, U, outcome and record -- under this rule.  Write L_H for the L above, H = levels, G_H = F_H.  For h = H .. 1:
 *   1. expand: G_(h-1) = the existing children of the nodes of G_h with U_(h-1) >= L_h.  At h = 1 they are the candidates and the search
 *      ends as above: the key maximum and the count of equals (L_0 = L_1)
 *   2. probe (h - 1 >= 1 and LSD_GRID_LOCATE_TIGHT_PROBE), per heading a: the node of G_(h-1) at heading a with the largest U_(h-1), among
 *      equals the smallest Q nbx_(h-1) + P (nbx_(h-1) = ceil(nx / 2^(h-1))) -- of the WHOLE set, the nodes that did not fit the list
 *      included; a heading without a node has no probe.  From it the greedy descent of the entry above, unchanged, ends at a candidate of
 *      score S_a.  L_(h-1) = max(L_h, max_a S_a); without the flag L_(h-1) = L_h
 *   3. retry (LSD_GRID_LOCATE_TIGHT_RETRY and |G_(h-1)| > max_nodes): G_(h-1) is rebuilt once, the children of G_h with U_(h-1) >= L_(h-1);
 *      the first count is kept in first_count[h-1] and bit h - 1 of `retried` is set.  No second probe follows
 *   4. OVERFLOW iff |G_(h-1)| > max_nodes for some h - 1 >= 1 after the retry where there was one, or |G_H| > max_nodes (no retry: no bound
 *      was raised yet).  The count is exact; the level and those below it are not run
 * Filtering is lazy: a node of G_(h-1) whose U is below a raised L_(h-1) stays and yields no children (a child's U never exceeds its
 * parent's), so the sets above ARE what the lists hold.  Correctness: every L_h is score_floor or the S of an existing candidate, so with
 * score_floor <= S_win every L_h <= S_win; every ancestor of a candidate that ties the winner has U >= S_win >= L_h and survives the
 * expansion and the retry: winner, n_best, outcome and pose are the exhaustive search's.
 * The record is lsd_grid_locate_rec; lower_bound = the last L_h reached.  The statistics (d_stats, may be NULL; 128 bytes per scan), whose
 * first 48 bytes read as lsd_grid_locate_stats: frontier[h] = |G_h| (a retried level: the second count);  scored = top_nodes + every child
 * evaluated, a retried level's twice;  retried;  bound[h] = L_h for h <= H, 0 above H and below an overflow;  first_count[h] = the count
 * before a retry, else 0;  EMPTY: all 0.
 * tight = 0: every record byte and the first 48 statistics bytes are the entry's above; levels <= 1 has no probe and no retry, whatever
 * `tight`.
 * lsd_enqueue_grid_locate_tight_device: levels + 6 + max(levels - 1, 0) * (1 + probe + retry) launches, probe and retry 1 where the flag
 * is set: offsets, top level, bound, frontier seed, the tight words, one expansion per level, between two levels the level kernel and
 * with their flags the probes and the retry, pick.  A number fixed by par and tight, never by the data: a retry that is not needed is a
 * launch that returns.  Asynchronous on `stream`; the workspace (lsd_grid_locate_tight_workspace_bytes: the entry's above, 128 bytes per
 * scan and 8 per scan and heading) is the context's, the same buffer, grown before the first launch when needed -- that case alone
 * synchronises; no other allocation, copy or host wait.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: whatever the
 * entry above refuses; `tight` with a bit beyond the two flags; d_stats not 4-byte aligned.  n_scans == 0 launches nothing. */
#define LSD_GRID_LOCATE_TIGHT_PROBE 1u
#define LSD_GRID_LOCATE_TIGHT_RETRY 2u
typedef struct lsd_grid_locate_tight_stats {   /* 128 bytes */
    uint32_t top_nodes, frontier[9], scored, retried, bound[9], first_count[9], reserved[2];
} lsd_grid_locate_tight_stats;
size_t lsd_grid_locate_tight_workspace_bytes(int n_scans, int stride, lsd_grid_locate_par par);
int lsd_enqueue_grid_locate_tight_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_scans, int stride,
                                         lsd_map_param map_param, double range_max, const uint8_t *d_pyramid, lsd_grid_locate_par par,
                                         uint32_t tight, lsd_grid_locate_rec *d_out, lsd_grid_locate_tight_stats *d_stats, void *stream);
/* Host convenience: lsd_grid_locate with the tight entry in its place.  Blocking. */
int lsd_grid_locate_tight(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_scans, int stride, lsd_map_param map_param,
                          double range_max, const uint8_t *corr, lsd_grid_locate_par par, uint32_t tight, lsd_grid_locate_rec *out,
                          lsd_grid_locate_tight_stats *stats);

/* --- pose graph: keyframes, loop closures and their relaxation, so that a grid can be drawn again from moved poses ---------------- */
/* Every grid entry above enters a scan at one pose and that pose is final.  This section keeps what was entered where (nodes and their
 * scans), the constraints between the entries (edges), redistributes the error (a relaxation) and leaves the nodes as a d_poses argument
 * of pitch 64 for lsd_enqueue_grid_integrate_device, which draws the grid again (csrc/k_pgbuild.hip, csrc/k_posegraph.hip,
 * csrc/posegraph_dev.h; restated in tests/pose_graph_cases.py).  All records are caller-owned device memory, 8-byte
 * aligned; a pose is map pixels and degrees, the integration's.  fp64 without FMA; every sum runs ascending from 0.0 unless its
 * parentheses say otherwise; sin / cos are the integration's: (s, c)(a) = sincos(a / 180.0 * pi).
 *   wrap(v) = v - 360.0 * floor((v + 180.0) / 360.0)
 *   rel(p, q), q in the frame of p:  dx = q.x - p.x, dy = q.y - p.y, (s, c)(p.ang);  (c * dx + s * dy, c * dy - s * dx, wrap(q.ang - p.ang))
 *   comp(p, z):  (s, c)(p.ang);  (p.x + (c * z.x - s * z.y), p.y + (s * z.x + c * z.y), wrap(p.ang + z.ang))
 *   inv3(S): the cofactor form of lsd_enqueue_fa_carry_correct_device's step 5, failing where !(det > 0) or 1 / det is not finite
 * A graph: one lsd_pg_head, nodes_cap nodes, edges_cap edges.  n_nodes and n_edges are read and written ON THE DEVICE; every entry uses
 * min(max(n, 0), cap) of them.  The keyframe store: nodes_cap rows of store_stride readings and nodes_cap lengths, row k node k's scan;
 * lengths start at 0, so the rows past n_nodes are empty scans to the integration. */
typedef struct lsd_pg_head { int32_t n_nodes, n_edges; } lsd_pg_head;                                   /* 8 bytes */
typedef struct lsd_pg_node {               /* 64 bytes; its head is a pose, so an array of these IS a d_poses argument (pitch 64) */
    double x, y, ang;
    double raw[3];                         /* the pose the node was appended from */
    uint32_t flags; int32_t track;
    uint64_t reserved;
} lsd_pg_node;
#define LSD_PG_NODE_FIXED 1u
typedef struct lsd_pg_edge {               /* 96 bytes */
    int32_t i, j; uint32_t flags, reserved;
    double z[3];                           /* the pose of j in the frame of i: pixels, pixels, degrees */
    double info[6];                        /* the information matrix: xx, xy, yy, xa, ya, aa */
    double chi2;                           /* written by the relaxation */
} lsd_pg_edge;
#define LSD_PG_EDGE_DISABLED 1u
#define LSD_PG_EDGE_CLOSURE 2u
typedef struct lsd_pg_track { int32_t last, reserved; double raw[3]; } lsd_pg_track;                    /* 32 bytes; last = -1: empty */
/* lsd_enqueue_pg_append_device: keyframes and odometry edges.  n_cand candidate frames, their scans, lengths, stride and poses at a pitch
 * exactly as lsd_enqueue_grid_integrate_device reads them, decided IN ORDER against one track record d_track (track: the id its nodes
 * get).  Candidate t with pose q is DROPPED when the integration would skip its scan whole (q not finite, fabs(q.x + 1) < 1e-4, |q.x| or
 * |q.y| > 1048576) or d_lens[t] <= 0.  Else, with the track empty (last outside 0..n_nodes-1): it becomes node n_nodes at pose q, raw = q,
 * flags = LSD_PG_NODE_FIXED iff it is node 0, and no edge.  Else z = rel(track.raw, q); it is a keyframe iff z.x * z.x + z.y * z.y >=
 * min_dist * min_dist or fabs(z.ang) >= min_ang; a keyframe becomes node n_nodes at comp(pose[last], z) -- the last node's CURRENT pose,
 * moved or not --, raw = q, flags = 0, and the edge (last, new, z, info, flags 0, chi2 +0.0) is appended.  A new node's reserved word is
 * 0; track.last = new, track.raw = q; store row `new` receives the first min(stride, store_stride) readings of the scan row byte for byte
 * and the length min(d_lens[t], stride, store_stride).  A candidate that is no keyframe changes nothing.  A keyframe that finds n_nodes ==
 * nodes_cap sets LSD_PG_APPEND_NODES_FULL, one that needs an edge and finds n_edges == edges_cap sets LSD_PG_APPEND_EDGES_FULL; either
 * appends nothing, neither node nor edge, and leaves the track as it is.  Report: nodes and edges appended, candidates dropped, flags.
 * One launch of one workgroup (a lane decides, all lanes copy the row), no workspace, no allocation, no host wait.  LSD_ERR_INVALID
 * before anything is enqueued, outputs untouched: a null pointer (d_rep may be NULL); n_cand < 0; stride or store_stride outside 1..the
 * context's scan capacity; pose_pitch < 24 or not a multiple of 8; nodes_cap outside 1..16384, edges_cap outside 1..65536; min_dist,
 * min_ang or one of info[6] not finite, min_dist or min_ang negative; scans or store not 16-byte, a record array not 8-byte, lengths not
 * 4-byte aligned.  n_cand == 0 launches nothing. */
typedef struct lsd_pg_append_par { double min_dist, min_ang, info[6]; } lsd_pg_append_par;              /* 64 bytes */
typedef struct lsd_pg_append_rep { int32_t nodes, edges, dropped; uint32_t flags; } lsd_pg_append_rep;  /* 16 bytes */
#define LSD_PG_APPEND_NODES_FULL 1u
#define LSD_PG_APPEND_EDGES_FULL 2u
int lsd_enqueue_pg_append_device(lsd_ctx *ctx, const lsd_polar *d_scans, const int *d_lens, int n_cand, int stride, const void *d_poses,
                                 size_t pose_pitch, lsd_pg_head *d_head, lsd_pg_node *d_nodes, int nodes_cap, lsd_pg_edge *d_edges,
                                 int edges_cap, lsd_pg_track *d_track, int32_t track, lsd_polar *d_store, int *d_store_lens,
                                 int store_stride, lsd_pg_append_par par, lsd_pg_append_rep *d_rep /* may be NULL */, void *stream);
/* lsd_enqueue_pg_near_device: the loop candidate.  The query j = d_track->last, read on the device.  With j in 0..n_nodes-1 the
 * candidates are the nodes i <= j - gap with d2_i = dx * dx + dy * dy <= radius * radius, dx = x_i - x_j, dy = y_i - y_j; the anchor is the
 * candidate of the smallest d2, among equals the smallest i; with no candidate, or j outside the nodes, the anchor is -1.  It writes
 *   (a) d_rec: anchor, query = j, the number of candidates, d2 of the anchor (+0.0 without one)
 *   (b) d_sel[nodes_cap], packed poses (24 bytes): node k's pose iff anchor >= 0, |k - anchor| <= window and k <= j - gap; otherwise the
 *       "no pose" sentinel (-1.0, +0.0, +0.0).  Integrating the WHOLE store at d_sel draws the anchor's neighbourhood alone, without the
 *       host knowing the anchor
 *   (c) the query gathered into a batch of one row, as lsd_enqueue_fa_lost_gather_device gathers: with j in the nodes d_q_scan receives
 *       store row j (store_stride readings), d_q_len its length and d_q_pose node j's pose -- the sentinel without an anchor; with j
 *       outside the nodes d_q_len = 0, d_q_pose = the sentinel and the row keeps its bytes
 * One launch of one workgroup, no workspace, no atomics.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer;
 * nodes_cap outside 1..16384; store_stride outside 1..the context's scan capacity; gap < 1 or window < 0; radius not finite or negative;
 * the alignments of the append. */
typedef struct lsd_pg_near_rec { int32_t anchor, query, n_cand, reserved; double d2; } lsd_pg_near_rec; /* 24 bytes */
int lsd_enqueue_pg_near_device(lsd_ctx *ctx, const lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap,
                               const lsd_pg_track *d_track, const lsd_polar *d_store, const int *d_store_lens, int store_stride, int gap,
                               double radius, int window, lsd_pg_near_rec *d_rec, lsd_position *d_sel, lsd_polar *d_q_scan, int *d_q_len,
                               lsd_position *d_q_pose, void *stream);
/* lsd_enqueue_pg_closure_device: the edge from the response record r of the query matched against the anchor's neighbourhood.  The first
 * test that fires decides; each outcome is exactly one flag; report: edge = the new edge's index or -1, det as far as computed, else +0.0:
 *   1. anchor or query outside 0..n_nodes-1, or anchor == query: NO_ANCHOR
 *   2. r.flags: VALID clear, or NONE, EMPTY or MISMATCH set: NO_RESPONSE (the correction's step 4)
 *   3. r.x, r.y, r.ang or one of r.cov[0..5] not finite: NOT_FINITE
 *   4. R exactly as the correction's step 5 builds it from cov_scale, floor_xy, floor_ang; I = inv3(R); on failure SINGULAR
 *   5. n_edges == edges_cap: FULL
 *   6. APPENDED: the edge (anchor, query), z = rel(pose[anchor], (r.x, r.y, r.ang)), flags = LSD_PG_EDGE_CLOSURE, chi2 = +0.0, and the
 *      information turned into the anchor's frame, (s, c)(pose[anchor].ang):  T(r,0) = I(r,0) * c + I(r,1) * s,  T(r,1) = I(r,1) * c -
 *      I(r,0) * s,  T(r,2) = I(r,2);  J(0,q) = c * T(0,q) + s * T(1,q),  J(1,q) = c * T(1,q) - s * T(0,q),  J(2,q) = T(2,q);
 *      info = J(0,0), J(0,1), J(1,1), J(0,2), J(1,2), J(2,2);  n_edges += 1
 * One launch, one lane.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer (d_rep may be NULL); the caps as
 * above; a parameter not finite or negative; a pointer not 8-byte aligned. */
typedef struct lsd_pg_closure_par { double cov_scale, floor_xy, floor_ang; } lsd_pg_closure_par;        /* 24 bytes */
typedef struct lsd_pg_closure_rep { int32_t edge; uint32_t flags; double det; } lsd_pg_closure_rep;     /* 16 bytes */
enum { LSD_PG_CLOSURE_APPENDED = 1, LSD_PG_CLOSURE_NO_ANCHOR = 2, LSD_PG_CLOSURE_NO_RESPONSE = 4, LSD_PG_CLOSURE_NOT_FINITE = 8,
       LSD_PG_CLOSURE_SINGULAR = 16, LSD_PG_CLOSURE_FULL = 32 };
int lsd_enqueue_pg_closure_device(lsd_ctx *ctx, lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap, lsd_pg_edge *d_edges,
                                  int edges_cap, const lsd_pg_near_rec *d_near, const lsd_grid_response_rec *d_resp,
                                  lsd_pg_closure_par par, lsd_pg_closure_rep *d_rep /* may be NULL */, void *stream);
/* lsd_enqueue_pg_relax_device: Levenberg-Marquardt over SE(2), the linear step by conjugate gradients preconditioned with the inverse
 * 3 x 3 diagonal blocks.  n_graphs graphs in one launch, ONE WORKGROUP PER GRAPH: graph g is d_heads[g], d_nodes + g * nodes_cap, d_edges
 * + g * edges_cap, d_rep[g] and the workspace bytes from g * lsd_pg_workspace_bytes(nodes_cap, edges_cap) on.  N and E are its clamped
 * counts.
 * Edge e = (i, j, z, info) is SKIPPED (counted; its chi2 is +0.0) when it is DISABLED, i == j, i or j is outside 0..N-1, or one of z[3],
 * info[6] or the poses of i and j, as they are when the call begins, is not finite.  W is the symmetric matrix of info.  At poses p:
 *   (s, c)(a_i);  dx = x_j - x_i, dy = y_j - y_i;  e = ((c * dx + s * dy) - z[0], (c * dy - s * dx) - z[1], wrap((a_j - a_i) - z[2]))
 *   k = pi / 180.0;  A = [(-c, -s, k * (c * dy - s * dx)), (s, -c, k * ((-c) * dx - s * dy)), (0.0, 0.0, -1.0)]
 *   B = [(c, s, 0.0), (-s, c, 0.0), (0.0, 0.0, 1.0)]
 *   WA(r,q) = sum_t W(r,t) * A(t,q), WB likewise, We(r) = sum_t W(r,t) * e[t]     (every product is made, the zeros' too)
 *   Haa(r,q) = sum_t A(t,r) * WA(t,q), Hab(r,q) = sum_t A(t,r) * WB(t,q), Hbb(r,q) = sum_t B(t,r) * WB(t,q),
 *   ba(r) = sum_t A(t,r) * We(t), bb(r) = sum_t B(t,r) * We(t), chi2_e = sum_t e[t] * We(t)
 * A node's list holds its edges that are not skipped, in ASCENDING EDGE INDEX.  A node is FREE unless it is FIXED or singular (below).
 * REDUCTIONS have one shape, which depends on the element count n alone: s[t] = v[t] + v[t + 1024] + .. (left to right) for t < 1024 and
 * t < n, +0.0 for t >= n; then s[t] = s[t] + s[t + h] for t < h, h = 512, 256, .. 1; the result is s[0].  dot(u, v) over nodes reduces
 * d_n = sum_q u_n[q] * v_n[q]; chi2 reduces chi2_e over all E edges; the largest |delta| is a maximum and has no order.
 *   chi2 = the reduction at the nodes' poses;  chi2_before = chi2;  lambda = lambda0.  chi2 not finite: NOT_FINITE, nothing more is done.
 *   An outer iteration, while done < iters:
 *   1. the blocks of every edge at the current poses
 *   2. H_n = the sum over the list of n of Haa (n is the edge's i) or Hbb (its j), b_n of ba or bb
 *   3. D_n = H_n with D(r,r) = H(r,r) + lambda * H(r,r);  M_n = inv3(D_n).  A node that is not FIXED and fails is SINGULAR from here to the
 *      end of the call (a node without edges is one)
 *   4. PCG on D delta = -b over the free nodes; delta, r, z, p are +0.0 at every other node.  delta = 0;  r_n = -b_n;  z_n = M_n r_n;  p = z;
 *      rz = rz0 = dot(r, z);  thr = (cg_tol * cg_tol) * rz0.  While steps < cg_iters and !(rz <= thr):  q_n = D_n p_n, then along the list
 *      q_n = q_n + Hab p_j (n is the edge's i) or q_n + Hab^T p_i (its j);  pq = dot(p, q);  !(pq > 0): BREAKDOWN, the loop ends;  alpha = rz /
 *      pq;  delta = delta + alpha * p;  r = r - alpha * q;  z_n = M_n r_n;  rz' = dot(r, z);  beta = rz' / rz;  p = z + beta * p;  rz = rz';
 *      steps += 1
 *   5. trial poses: (x + delta[0], y + delta[1], wrap(ang + delta[2])) at a free node, the node's own bytes elsewhere;  chi2' = the
 *      reduction at the trial poses;  done += 1.  chi2' <= chi2: ACCEPTED -- the trial poses become the poses, chi2 = chi2', lambda =
 *      max(lambda / down, lambda_min), and with max |delta[q]| over all nodes < eps: CONVERGED, the loop ends.  Otherwise REJECTED: lambda =
 *      lambda * up
 * Outputs: the nodes' x, y, ang in place, every other byte of a node kept; edge.chi2 = chi2_e at the final poses; the report: chi2_before,
 * chi2_after = chi2, the last lambda, outer iterations done, CG steps summed, steps accepted and rejected, edges skipped, nodes singular,
 * flags.  iters == 0 computes chi2 and edge.chi2 only.
 * Asynchronous on `stream`, one launch of n_graphs workgroups; every loop is bounded by a parameter and no workgroup waits for another.
 * The lists are built on the device once per call (count, scan, fill, order).  The workspace is the caller's; no allocation, no atomics
 * on fp64, no host wait.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; n_graphs < 0; nodes_cap outside
 * 1..16384, edges_cap outside 1..65536; a parameter not finite or negative; up <= 1, down < 1; iters or cg_iters outside 0..65535; a pointer
 * not 8-byte aligned.  n_graphs == 0 launches nothing.  lsd_pg_workspace_bytes: 0 for caps outside the limits. */
typedef struct lsd_pg_relax_par {          /* 56 bytes */
    double lambda0, lambda_min, up, down, cg_tol, eps; int32_t iters, cg_iters;
} lsd_pg_relax_par;
typedef struct lsd_pg_relax_rep {          /* 56 bytes */
    double chi2_before, chi2_after, lambda;
    int32_t iters, cg_iters, accepted, rejected, skipped_edges, singular_nodes; uint32_t flags, reserved;
} lsd_pg_relax_rep;
#define LSD_PG_RELAX_CONVERGED 1u
#define LSD_PG_RELAX_BREAKDOWN 2u
#define LSD_PG_RELAX_NOT_FINITE 4u
size_t lsd_pg_workspace_bytes(int nodes_cap, int edges_cap);
int lsd_enqueue_pg_relax_device(lsd_ctx *ctx, int n_graphs, const lsd_pg_head *d_heads, lsd_pg_node *d_nodes, int nodes_cap,
                                lsd_pg_edge *d_edges, int edges_cap, lsd_pg_relax_par par, void *d_workspace, lsd_pg_relax_rep *d_rep,
                                void *stream);
/* lsd_enqueue_pg_relax_robust_device: the relaxation above with a robust kernel on its edges, so that a closure that is confidently wrong
 * loses its pull instead of bending the graph (csrc/k_posegraph.hip, the same body compiled a second time; restated in
 * tests/pose_graph_robust_cases.py).  The arguments of lsd_enqueue_pg_relax_device, the kernel `rob` and one lsd_pg_robust_rep per graph
 * (d_rob_rep may be NULL).  Everything that is not named here is the text above, word for word: the skipping of edges, the lists, the one
 * reduction shape, PCG, the singular nodes, the stops.
 *   An edge is IN SCOPE when it is not skipped and either scope == LSD_PG_ROBUST_ALL or LSD_PG_EDGE_CLOSURE is set.
 *   s = chi2_e, the plain value at the poses in question;  c = delta * delta.  The weight w and the cost rho of an edge:
 *     out of scope, or kernel NONE:  w = 1.0, rho = s
 *     HUBER:  s <= c:  w = 1.0, rho = s;  otherwise  r = sqrt(s), w = delta / r, rho = (2.0 * delta) * r - c      (sqrt of a NaN: that NaN)
 *     GM (Geman-McClure):  t = c / (c + s), w = t * t, rho = (c * s) / (c + s)
 *     a skipped edge:  rho = +0.0
 *   The objective F = the reduction over all E edges of rho_e stands wherever the plain rule says chi2: the value at the start (not finite:
 *   NOT_FINITE, nothing more is done), the test F' <= F at the trial poses, chi2_before and chi2_after of the lsd_pg_relax_rep.
 *   Step 1: w_e at the current poses; W'(r,t) = w_e * W(r,t) -- all nine products, also when w_e is 1.0 --; WA, WB and the We of ba and bb
 *   come from W'; chi2_e itself comes from W.  Multiplying by 1.0 is exact: kernel NONE, and HUBER with a delta above every sqrt(chi2_e)
 *   met, give the bytes of lsd_enqueue_pg_relax_device.
 * Outputs: the nodes in place; edge.chi2 = the PLAIN chi2_e at the final poses (lsd_enqueue_pg_prune_device reads it); d_rep as above with
 * F in the place of chi2; d_rob_rep: chi2_plain = the reduction of those plain values; downweighted = the edges in scope with w < 1.0 at the
 * final poses; w_min = the smallest w among the edges in scope and w_min_edge the smallest index that has it -- 1.0 and -1 when no edge is
 * in scope; when some w is a NaN, that NaN and the smallest index that holds one.  (A NaN that the device makes out of finite numbers is
 * the quiet one with the sign set, 0xfff8000000000000, and no operation of the rule turns its sign; an input that is not finite is skipped.)
 * The workspace is lsd_pg_workspace_bytes per graph: a weight is made again from chi2_e where it is needed and never stored.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: everything lsd_enqueue_pg_relax_device refuses; kernel outside 0..2;
 * scope outside 0..1; with kernel != NONE a delta that is not finite or not > 0; d_rob_rep not 8-byte aligned. */
typedef struct lsd_pg_robust_par { int32_t kernel; uint32_t scope; double delta; } lsd_pg_robust_par;   /* 16 bytes */
enum { LSD_PG_KERNEL_NONE = 0, LSD_PG_KERNEL_HUBER = 1, LSD_PG_KERNEL_GM = 2 };
enum { LSD_PG_ROBUST_CLOSURES = 0, LSD_PG_ROBUST_ALL = 1 };
typedef struct lsd_pg_robust_rep { double chi2_plain, w_min; int32_t downweighted, w_min_edge; } lsd_pg_robust_rep;  /* 24 bytes */
int lsd_enqueue_pg_relax_robust_device(lsd_ctx *ctx, int n_graphs, const lsd_pg_head *d_heads, lsd_pg_node *d_nodes, int nodes_cap,
                                       lsd_pg_edge *d_edges, int edges_cap, lsd_pg_relax_par par, lsd_pg_robust_par rob, void *d_workspace,
                                       lsd_pg_relax_rep *d_rep, lsd_pg_robust_rep *d_rob_rep /* may be NULL */, void *stream);
/* lsd_enqueue_pg_relax_pc_device: the robust relaxation above with a choice of preconditioner (csrc/k_pgchain.hip, csrc/pgrelax_dev.h: the
 * same body compiled a third time; restated in tests/pose_graph_chain_cases.py).  The arguments of
 * lsd_enqueue_pg_relax_robust_device, `pc` and one lsd_pg_precond_rep per graph (d_pc_rep may be NULL).  The workspace of graph g begins at
 * g * lsd_pg_workspace_pc_bytes(nodes_cap, edges_cap, pc.kind).
 * kind BLOCK launches lsd_enqueue_pg_relax_robust_device's kernel and gives its bytes (with kernel NONE those of
 * lsd_enqueue_pg_relax_device); every d_pc_rep[g] is zeros.
 * kind CHAIN: M is the block-tridiagonal part of the damped normal matrix D along the graph's odometry chains, and z = M^-1 r stands
 * wherever the rule says z_n = M_n r_n.  A track's graph is a chain plus a few closures, D differs from M by the closures' off-diagonal
 * blocks alone, and PCG needs a number of steps that follows the closures, not the length of the track.  Everything that is not named
 * here is the text of the two entries above, word for word: the skipping of edges, the lists, the weights, the one reduction shape, the
 * singular and fixed nodes, PCG, BREAKDOWN, the stops.  fp64 without FMA, every sum left to right from +0.0, no atomics on fp64.
 *   CHAIN EDGES, once per call, integers only.  A CANDIDATE is an edge that is not skipped and has LSD_PG_EDGE_CLOSURE clear; lo = min(i, j),
 *   hi = max(i, j); up[n] = the smallest candidate index whose lo is n, down[n] = the smallest whose hi is n.  Edge e is a CHAIN edge iff
 *   up[lo(e)] == e and down[hi(e)] == e.  No order of the edges enters.  A node has at most one chain edge upwards and one downwards, so
 *   the chain edges form disjoint PATHS with ascending node indices; a node's RANK is its distance from its path's head (the node with no
 *   chain edge downwards); a node on no chain edge is a path of one.
 *   POSITIONS t = 0 .. N-1: the paths one after another in ascending head index, each in rank order; node(t) is the node at t.
 *   BLOCKS, per outer iteration behind step 3.  Dg[t] = D_n of node(t) where it is FREE, the identity elsewhere.  C[t], t < N-1, rows
 *   belonging to node(t): where a chain edge e joins node(t) and node(t+1) and both are free, e's Hab (node(t) is e.i) or Hab transposed
 *   (node(t) is e.j) -- the weighted blocks of step 1 --; every entry +0.0 elsewhere.
 *   FACTOR, block cyclic reduction.  Levels s = 1, 2, 4, .. while s < N.  At a level every t with t mod 2s == s is eliminated; a = t - s,
 *   c = t + s; L = the current coupling (a, t), R = the current coupling (t, c) where c < N (at s = 1 they are C[a] and C[t]):
 *     P_t = inv3(Dg[t]);  GL_t(r,q) = sum_u L(r,u) * P_t(u,q);  with c < N: GU_t(r,q) = sum_u R(u,r) * P_t(u,q)
 *     Dg[a](r,q) = Dg[a](r,q) - sum_u GL_t(r,u) * L(q,u);  with c < N: Dg[c](r,q) = Dg[c](r,q) - sum_u GU_t(r,u) * R(u,q)
 *     with c < N the new coupling (a, c)(r,q) = -(sum_u GL_t(r,u) * R(u,q))
 *   A position that receives from both sides at one level takes the lower side (t = c' - s) first, the upper side (t = c' + s) second.
 *   Dg[t] is read as it stands when t's level begins.  Position 0 is never eliminated: P_0 = inv3(Dg[0]) behind the last level.
 *   APPLY.  y[t] = r of node(t).  Forward over the same levels, a position again taking the lower side first:
 *     y[c](r) = y[c](r) - sum_q GU_t(r,q) * y[t](q);  y[a](r) = y[a](r) - sum_q GL_t(r,q) * y[t](q)
 *   x[0](r) = sum_q P_0(r,q) * y[0](q).  Backward, s descending over the same levels, L and R as they were when t was eliminated:
 *     v(r) = y[t](r) - sum_q L(q,r) * x[a](q);  with c < N: v(r) = v(r) - sum_q R(r,q) * x[c](q);  x[t](r) = sum_q P_t(r,q) * v(q)
 *   z of node(t) = x[t] where it is free, +0.0 elsewhere.
 *   FALLBACK.  Where an inv3 of the factor fails, this outer iteration runs on the Jacobi blocks M_n exactly as the plain rule does -- its
 *   bytes are the plain rule's -- and `fallbacks` counts it.  (M is symmetric positive definite for information matrices that are: the sum
 *   of the chain edges' own terms, the diagonal blocks of all other edges and lambda * diag(H).)
 * d_pc_rep: the chain edges, the paths (those of one node too), the nodes of the longest path, the outer iterations that fell back; all 0
 * for N == 0.  iters == 0 still reports the chain.
 * One launch, ONE WORKGROUP PER GRAPH; ranks by pointer doubling, up and down by integer atomics; no allocation, no host wait.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: everything lsd_enqueue_pg_relax_robust_device refuses; kind outside 0..1;
 * reserved != 0; d_pc_rep not 8-byte aligned.  lsd_pg_workspace_pc_bytes: lsd_pg_workspace_bytes for BLOCK; for CHAIN that plus the
 * factor's planes and the positions (51 doubles and 6 words per node, rounded up to 256 bytes); 0 for caps outside the limits or a kind
 * outside 0..1. */
typedef struct lsd_pg_precond_par { int32_t kind; int32_t reserved; } lsd_pg_precond_par;               /* 8 bytes */
enum { LSD_PG_PRECOND_BLOCK = 0, LSD_PG_PRECOND_CHAIN = 1 };
typedef struct lsd_pg_precond_rep { int32_t chain_edges, paths, longest_path, fallbacks; } lsd_pg_precond_rep;   /* 16 bytes */
size_t lsd_pg_workspace_pc_bytes(int nodes_cap, int edges_cap, int kind);
int lsd_enqueue_pg_relax_pc_device(lsd_ctx *ctx, int n_graphs, const lsd_pg_head *d_heads, lsd_pg_node *d_nodes, int nodes_cap,
                                   lsd_pg_edge *d_edges, int edges_cap, lsd_pg_relax_par par, lsd_pg_robust_par rob, lsd_pg_precond_par pc,
                                   void *d_workspace, lsd_pg_relax_rep *d_rep, lsd_pg_robust_rep *d_rob_rep /* may be NULL */,
                                   lsd_pg_precond_rep *d_pc_rep /* may be NULL */, void *stream);
/* lsd_enqueue_pg_prune_device: closures whose chi2 -- the last relaxation's -- is beyond a gate are taken out of the graph, on the device
 * (csrc/k_pgprune.hip).  Graph g is d_heads[g], d_edges + g * edges_cap and d_rep[g]; E is its clamped n_edges.
 *   A CANDIDATE is an edge e < E with CLOSURE set, DISABLED clear and !(chi2 <= gate): a NaN is one.
 *   Candidates are ordered by chi2 descending, a NaN counting as +infinity, equals by ascending index.
 *   The first min(max_reject, candidates) of that order get flags |= LSD_PG_EDGE_DISABLED | LSD_PG_EDGE_REJECTED.  No other byte of any
 *   edge changes; nothing at or beyond E changes.
 *   Report: candidates; rejected; worst_edge and worst_chi2 = the first of the order, its chi2 as it stands (-1 and +0.0 without a
 *   candidate); closures_left = the CLOSURE edges below E that are not DISABLED afterwards.  max_reject == 0 only counts.
 * One launch, ONE WORKGROUP PER GRAPH: at most max(max_reject, 1) rounds of one arg-max each, no workspace, no atomics on fp64, no host
 * wait.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; n_graphs < 0; edges_cap outside 1..65536; gate not
 * finite or negative; max_reject outside 0..64; a pointer not 8-byte aligned.  n_graphs == 0 launches nothing. */
typedef struct lsd_pg_prune_par { double gate; int32_t max_reject, reserved; } lsd_pg_prune_par;        /* 16 bytes */
typedef struct lsd_pg_prune_rep { int32_t candidates, rejected, worst_edge, closures_left; double worst_chi2; } lsd_pg_prune_rep; /* 24 bytes */
#define LSD_PG_EDGE_REJECTED 4u
int lsd_enqueue_pg_prune_device(lsd_ctx *ctx, int n_graphs, const lsd_pg_head *d_heads, lsd_pg_edge *d_edges, int edges_cap,
                                lsd_pg_prune_par par, lsd_pg_prune_rep *d_rep, void *stream);
/* lsd_enqueue_pg_marginals_device: marginal covariances of ONE graph -- of a node, of one node relative to another, of the two ends of an
 * edge that was appended since a copy of the head was taken -- by solves with the relaxation's normal matrix (csrc/k_pgmarg.hip; DESIGN.md
 * 8.1.20; restated in tests/pose_graph_marginal_cases.py).  Nothing of the graph changes.  fp64 without FMA, every sum left to right from
 * +0.0, no atomics on fp64, the one reduction shape wherever a dot product is reduced.  Everything that is not named here is the text of
 * lsd_enqueue_pg_relax_device and lsd_enqueue_pg_relax_pc_device, word for word.
 *   THE MATRIX.  N and E are the clamped counts of d_head.  E_h = E without d_prior; with it E_h = min(E, clamp(d_prior->n_edges)), the
 *   clamp being min(max(., 0), edges_cap), read on the device: the matrix is the graph as it stood when d_prior was copied, so that the
 *   edges appended since do not vouch for themselves.  Only the edges e < E_h exist for the matrix; they are skipped exactly as the
 *   relaxation skips them.  The blocks are those of the relaxation's step 1 at the nodes' poses with plain weights (no robust kernel),
 *   H_n is step 2's, lambda = 0.0: D(r,r) = H(r,r) + 0.0 * H(r,r), M_n = inv3(D_n).  A node is FIXED or SINGULAR as there (a node without
 *   an edge below E_h is singular).  precond CHAIN: the chain edges, positions, blocks and factor of lsd_enqueue_pg_relax_pc_device over the
 *   edges e < E_h at lambda = 0.0; where an inv3 of the factor fails the WHOLE call runs on the Jacobi blocks and fallbacks = 1.
 *   A QUERY is {kind, a, b}.  U is a right-hand side of three columns over the nodes, +0.0 at every node that is not free.
 *     NODE (a): a outside 0..N-1: BAD_QUERY.  a FIXED: the flag FIXED; a SINGULAR: the flag SINGULAR; neither is solved.  Else column c
 *       of U is the unit vector c at node a, and cov(r,c) = x_c[a][r].
 *     PAIR (a, b): a or b outside 0..N-1, or a == b: BAD_QUERY.  With (s, c), dx, dy, A and B of the relaxation's rule for an edge (i = a,
 *       j = b) at the nodes' poses: column c of U is row c of A at node a and row c of B at node b, the part of a node that is not free
 *       dropped (the flags FIXED and SINGULAR say that some end is; the solves are made all the same).
 *       cov(r,c) = (sum_q A(r,q) * x_c[a][q]) + (sum_q B(r,q) * x_c[b][q]), every product made, x being +0.0 at a node that is not free:
 *       the covariance of rel(pose_a, pose_b) in pixels, pixels and degrees, in the frame of a.
 *     NEW_EDGE (k = a): without d_prior, or k < 0: BAD_QUERY.  e = clamp(d_prior->n_edges) + k; e >= E: NO_EDGE.  Else the PAIR
 *       (edges[e].i, edges[e].j), both read on the device.
 *     Any other kind: BAD_QUERY.
 *   THE SOLVE, column after column, c = 0, 1, 2: PCG on H x = u exactly as step 4 of the relaxation with u in the place of -b: x = 0;
 *   r = u; z = M^-1 r (z_n = M_n r_n, or the chain's apply); p = z; rz = rz0 = dot(r, z); thr = (cg_tol * cg_tol) * rz0; while steps <
 *   cg_iters and !(rz <= thr): the step of the relaxation; !(pq > 0) ends the column as BREAKDOWN.  A column that ends with rz <= thr is
 *   CONVERGED (rz0 == 0: with 0 steps and x = 0), one that ends otherwise without a breakdown is MAXED: exactly one of the three per column.
 *   THE RECORD: cov[3 * r + c] as computed -- NOT symmetrised --, +0.0 nine times where nothing was solved; steps[c]; flags; the query's
 *   kind; edge = e for NEW_EDGE with a prior and k >= 0 (also when NO_EDGE; beyond int32: 2147483647), else -1; i, j = the two nodes (a
 *   and b as given for NODE and PAIR; -1, -1 where NEW_EDGE found no edge).
 *   A GRAPH WITHOUT A FIXED NODE (or a component that no edge joins to one) has a singular matrix.  Its columns usually end MAXED or in
 *   BREAKDOWN, but nothing in the rule forbids CONVERGED: with CHAIN the factor of the singular matrix need not fail, z is then enormous
 *   along the free directions, rz0 with it, and the relative stop is met -- the covariance that comes out is enormous, not small, and
 *   lsd_enqueue_pg_vet_device passes every closure on it: the gate is vacuous on such a graph.  Fix a node.
 *   INDEPENDENCE: a record depends on the graph, d_prior and its query alone -- not on n_q, on slots, on its place in d_queries or on the
 *   workgroup that served it.
 *   THE REPORT: n_nodes = N, n_edges = E_h, the edges skipped among them, the singular nodes, the chain's three counts (0 for BLOCK),
 *   fallbacks.
 * Two launches on `stream`: the matrix by one workgroup into the shared part of the workspace, then min(n_q, slots) workgroups of which
 * workgroup s serves the queries s, s + slots, .. with its vectors in slice s.  Every loop is bounded by a parameter, no workgroup waits
 * for another, no allocation, no host wait.  lsd_pg_marginals_workspace_bytes = lsd_pg_workspace_pc_bytes(nodes_cap, edges_cap, precond)
 * + slots slices of 15 (BLOCK) or 21 (CHAIN) doubles per node of nodes_cap, each rounded up to 256 bytes; 0 for arguments outside the limits.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer other than d_prior (d_queries and d_recs may be null
 * with n_q == 0); the caps of the relaxation; cg_tol not finite or negative; cg_iters outside 0..65535; precond outside 0..1; slots
 * outside 1..1024; reserved != 0; n_q outside 0..65536; a pointer not 8-byte aligned.  n_q == 0 launches nothing and writes nothing. */
typedef struct lsd_pg_marg_query { int32_t kind, a, b, reserved; } lsd_pg_marg_query;                   /* 16 bytes */
enum { LSD_PG_MARG_NODE = 0, LSD_PG_MARG_PAIR = 1, LSD_PG_MARG_NEW_EDGE = 2 };
typedef struct lsd_pg_marg_par { double cg_tol; int32_t cg_iters, precond, slots, reserved; } lsd_pg_marg_par;   /* 24 bytes */
typedef struct lsd_pg_marg_rec {           /* 104 bytes */
    double cov[9]; int32_t steps[3]; uint32_t flags; int32_t kind, edge, i, j;
} lsd_pg_marg_rec;
#define LSD_PG_MARG_CONVERGED_0 0x1u       /* column c: << c */
#define LSD_PG_MARG_MAXED_0 0x10u
#define LSD_PG_MARG_BREAKDOWN_0 0x100u
#define LSD_PG_MARG_CONVERGED 0x7u         /* all three columns */
#define LSD_PG_MARG_FIXED 0x1000u
#define LSD_PG_MARG_SINGULAR 0x2000u
#define LSD_PG_MARG_BAD_QUERY 0x4000u
#define LSD_PG_MARG_NO_EDGE 0x8000u
typedef struct lsd_pg_marg_rep {           /* 32 bytes */
    int32_t n_nodes, n_edges, skipped_edges, singular_nodes, chain_edges, paths, longest_path, fallbacks;
} lsd_pg_marg_rep;
size_t lsd_pg_marginals_workspace_bytes(int nodes_cap, int edges_cap, int precond, int slots);
int lsd_enqueue_pg_marginals_device(lsd_ctx *ctx, const lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap,
                                    const lsd_pg_edge *d_edges, int edges_cap, const lsd_pg_head *d_prior /* may be NULL */,
                                    const lsd_pg_marg_query *d_queries, int n_q, lsd_pg_marg_par par, void *d_workspace,
                                    lsd_pg_marg_rec *d_recs, lsd_pg_marg_rep *d_rep, void *stream);
/* lsd_enqueue_pg_vet_device: the gate on new closures -- is a closure's error at the current poses plausible, given what the graph knew
 * of its two nodes before it?  d_queries[n_q] and d_recs[n_q] are those of lsd_enqueue_pg_marginals_device; N and E are d_head's clamped
 * counts.  A query whose kind is not NEW_EDGE is not looked at: UNUSED.  For the others the first test that fires decides, and the outcome
 * is exactly one flag:
 *   1. the record says NO_EDGE or BAD_QUERY, or its edge is outside 0..E-1: NO_EDGE
 *   2. edge e = the record's edge, as it stands when the launch begins: CLOSURE clear, DISABLED set, or skipped by the relaxation (i == j,
 *      i or j outside 0..N-1, z, info or the two poses not finite): SKIPPED
 *   3. the record is not CONVERGED in all three columns: NO_MARGINAL -- an unknown covariance rejects nothing
 *   4. R = inv3(W), W the symmetric matrix of the edge's info, fails: SINGULAR, det = det(W)
 *   5. S[q] = cov[q] + R[q] for q = 0..8 (not symmetrised); inv3(S) fails: SINGULAR, det = det(S)
 *   6. e = the edge's error at the current poses; t(r) = sum_q S^-1(r,q) * e[q]; d2 = sum_r e[r] * t(r); det = det(S).  !(d2 <= gate), a NaN
 *      included: REJECTED -- flags |= LSD_PG_EDGE_DISABLED | LSD_PG_EDGE_REJECTED, the bits the prune sets, and no other byte of any edge
 *      changes
 *   7. otherwise PASSED
 * d_rep[q] (d_rep may be NULL): d2 and det (+0.0 where the test that computes them was not reached), the edge (-1 for UNUSED and NO_EDGE)
 * and the flag.  Every outcome is decided from the edges as they stand when the launch begins and the bits are set behind that, so two
 * queries that name one edge decide alike and write the same bits.  One launch of ONE workgroup, a lane per query and round, no
 * workspace, no host wait.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer other than d_rep (d_queries
 * and d_recs may be null with n_q == 0); the caps of the relaxation; gate not finite or negative; n_q outside 0..65536; a pointer not
 * 8-byte aligned.  n_q == 0 launches nothing. */
typedef struct lsd_pg_vet_rep { double d2, det; int32_t edge; uint32_t flags; } lsd_pg_vet_rep;         /* 24 bytes */
enum { LSD_PG_VET_UNUSED = 1, LSD_PG_VET_NO_EDGE = 2, LSD_PG_VET_SKIPPED = 4, LSD_PG_VET_NO_MARGINAL = 8, LSD_PG_VET_SINGULAR = 16,
       LSD_PG_VET_REJECTED = 32, LSD_PG_VET_PASSED = 64 };
int lsd_enqueue_pg_vet_device(lsd_ctx *ctx, const lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap, lsd_pg_edge *d_edges,
                              int edges_cap, const lsd_pg_marg_query *d_queries, const lsd_pg_marg_rec *d_recs, int n_q, double gate,
                              lsd_pg_vet_rep *d_rep /* may be NULL */, void *stream);
/* Place recognition: loop candidates by the APPEARANCE of a keyframe's scan instead of its drifted pose, so that a loop is found when
 * lsd_enqueue_pg_near_device's radius no longer reaches (csrc/k_pgplace.hip; restated in
 * tests/pose_graph_place_cases.py).  One quantisation in fp64 without FMA, integers from there on.
 * lsd_enqueue_pg_describe_device: one lsd_pg_desc per keyframe.  N = min(max(d_head->n_nodes, 0), nodes_cap), read on the device.  Every
 * row k < N with d_desc[k].valid == 0 is described; a row with valid != 0 and every row >= N keep their bytes, so the launch needs no count
 * from the host and may be repeated freely (a store of zeroed records is "nothing described yet").  Row k:
 *   1. len = min(max(d_store_lens[k], 0), store_stride); the readings d_store[k * store_stride + 0..len-1]
 *   2. a reading is USED iff range is finite, range > 0, range <= range_max and angle is finite (the integration's hit test)
 *   3. its sector: t = angle / 6.283185307179586; f = t - floor(t); s = (int)(f * 64.0); s > 63 becomes 63 (f == 1.0 from a tiny negative
 *      angle)
 *   4. its value: q = (int)(range / range_max * 255.0); q > 254 becomes 254
 *   5. per sector, in uint32: sum[s] += q, cnt[s] += 1 (no order: integers)
 *   6. v[s] = cnt[s] ? sum[s] / cnt[s] : 255 (no return reads as "farther than range_max"); n_hits = the sum of cnt; n_sectors = the number
 *      of sectors with cnt > 0; valid = 1
 * One launch, one workgroup per row (a grid-stride over the rows), every row written by exactly one workgroup: no counter, no workspace.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; nodes_cap outside 1..16384; store_stride outside 1..the
 * context's scan capacity; range_max not finite or not > 0; d_store not 16-byte, d_head or d_desc not 8-byte, d_store_lens not 4-byte
 * aligned. */
#define LSD_PG_DESC_SECTORS 64
#define LSD_PG_PLACE_MAX 8
typedef struct lsd_pg_desc { uint8_t v[LSD_PG_DESC_SECTORS]; uint32_t n_hits; uint16_t n_sectors, valid; } lsd_pg_desc;   /* 72 bytes */
int lsd_enqueue_pg_describe_device(lsd_ctx *ctx, const lsd_pg_head *d_head, int nodes_cap, const lsd_polar *d_store,
                                   const int *d_store_lens, int store_stride, double range_max, lsd_pg_desc *d_desc, void *stream);
/* lsd_enqueue_pg_recognize_device: the places a query looks like.  The distance of a query a and a candidate c:
 *   D_s = sum over k = 0..63 of |a.v[(k + s) mod 64] - c.v[k]|, s = 0..63;  dist = the smallest D_s;  shift = the smallest s that has it
 * The query j = d_track->last and N (as above) are read on the device.  The query is USABLE iff j is in 0..N-1, d_desc[j].valid != 0 and
 * d_desc[j].n_sectors >= min_sectors.  Node i is a CANDIDATE iff the query is usable, i <= j - gap, d_desc[i].valid != 0,
 * d_desc[i].n_sectors >= min_sectors and dist_i <= max_dist; n_cand counts them.
 *   d_work[i], i < N: (dist_i << 6) | shift_i of a candidate, 0xffffffff of every other node; d_work[i], i >= N, keeps its bytes.
 *   Rounds r = 0..k-1: the candidate that is not suppressed with the smallest (dist, i) becomes d_recs[r] = (anchor, shift, dist, 0) and
 *   suppresses every i' with |i' - anchor| <= spread for the later rounds; a round without a candidate writes (-1, 0, 0, 0).  n_picked is
 *   the number of rounds filled.  d_rep = (query = j, n_cand, n_picked, 0).
 *   With A = d_recs[pick].anchor the outputs d_near, d_sel, d_q_scan, d_q_len and d_q_pose are written exactly as
 *   lsd_enqueue_pg_near_device writes them for the anchor A (its (a), (b), (c), every "no anchor" and "no query" case included), but
 *   d_near->d2 = (double)dist (+0.0 without an anchor), d_near->n_cand = n_cand, and with A >= 0
 *   d_q_pose = (x_A, y_A, wrap(ang_A - shift * 5.625)):  a direction at angle th in the anchor's frame is seen at th + shift * 5.625 degrees
 *   in the query's, so the query's heading is the anchor's MINUS the shift.  The match that follows searches around the anchor's pose
 *   turned that way, not around the query's drifted one.
 * Two launches: one scores (many workgroups, a grid-stride over i, one lane per candidate, integers only), one of one workgroup does the
 * rounds, the records, d_sel and the gather.  d_work: nodes_cap uint32 of the caller's.  No host wait, no allocation, no workgroup waits
 * for another.  LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; nodes_cap outside 1..16384; store_stride
 * outside 1..the context's scan capacity; gap < 1; window < 0 or spread < 0; k outside 1..LSD_PG_PLACE_MAX; pick outside 0..k-1; max_dist >
 * 16320; min_sectors outside 1..64; d_store or d_q_scan not 16-byte, a record array or d_desc not 8-byte, d_store_lens, d_q_len or d_work
 * not 4-byte aligned. */
typedef struct lsd_pg_place_par { int32_t gap, window, spread, k, pick; uint32_t max_dist, min_sectors, reserved; } lsd_pg_place_par; /* 32 bytes */
typedef struct lsd_pg_place_rec { int32_t anchor, shift; uint32_t dist, reserved; } lsd_pg_place_rec;   /* 16 bytes */
typedef struct lsd_pg_place_rep { int32_t query, n_cand, n_picked, reserved; } lsd_pg_place_rep;        /* 16 bytes */
int lsd_enqueue_pg_recognize_device(lsd_ctx *ctx, const lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap,
                                    const lsd_pg_track *d_track, const lsd_polar *d_store, const int *d_store_lens, int store_stride,
                                    const lsd_pg_desc *d_desc, lsd_pg_place_par par, uint32_t *d_work, lsd_pg_place_rec *d_recs,
                                    lsd_pg_place_rep *d_rep, lsd_pg_near_rec *d_near, lsd_position *d_sel, lsd_polar *d_q_scan,
                                    int *d_q_len, lsd_position *d_q_pose, void *stream);
/* Every loop of a track in one pass (csrc/k_pgloops.hip; restated in tests/pose_graph_loops_cases.py): the entry above
 * asks for ONE keyframe, the track's last; these three ask for a range of them, choose the distinct loops among the answers and hand each
 * to the closure chain, all on the device.  Integers only.
 * lsd_enqueue_pg_recognize_all_device: the keyframes q_lo .. q_lo + n_q - 1 as queries in one launch.  For q = 0..n_q-1, j = q_lo + q:
 *   d_recs[q * k .. q * k + k - 1] and d_reps[q] receive exactly the bytes lsd_enqueue_pg_recognize_device writes to d_recs and d_rep when
 *   d_track->last == j: N clamped on the device, the usability test, the candidates i <= j - gap, (dist, shift) with the smallest shift
 *   among equals, k rounds with `spread`, (-1, 0, 0, 0) for a round without a candidate, and the report of a j outside the nodes
 *   (query = j, no candidate, nothing picked).  No near record, selection or gather; par.pick and par.window are checked and not used.
 * One launch, ONE WORKGROUP PER QUERY, the heaviest (largest j) first; the keys of a query live in the workgroup's LDS (nodes_cap words) in
 * the place of d_work: no workspace.  Every loop is bounded by a parameter, no workgroup waits for another, no host wait.
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; nodes_cap outside 1..16384; the parameters the entry
 * above refuses; q_lo < 0, n_q < 0 or q_lo + n_q > nodes_cap; d_head, d_desc, d_recs or d_reps not 8-byte aligned.  n_q == 0 launches
 * nothing. */
int lsd_enqueue_pg_recognize_all_device(lsd_ctx *ctx, const lsd_pg_head *d_head, int nodes_cap, const lsd_pg_desc *d_desc,
                                        lsd_pg_place_par par, int q_lo, int n_q, lsd_pg_place_rec *d_recs /* n_q * par.k */,
                                        lsd_pg_place_rep *d_reps /* n_q */, void *stream);
/* lsd_enqueue_pg_loops_device: the distinct loops among the records d_recs[n_q * k], d_reps[n_q] that the entry above left for (q_lo,
 * n_q, k), given the closures the graph already has (d_head, d_edges; E = min(max(n_edges, 0), edges_cap), read on the device).
 *   A PAIR is a record with anchor >= 0; its query is d_reps[q].query.  n_pairs counts them.
 *   A pair (q, a) is KNOWN iff some edge e < E has LSD_PG_EDGE_CLOSURE set, |q - max(e.i, e.j)| <= spread and |a - min(e.i, e.j)| <=
 *   spread -- DISABLED and REJECTED or not.  n_known counts them; a known pair takes no part in the rounds.
 *   Rounds m = 0..max_loops-1: among the pairs neither known nor suppressed the one with the smallest (dist, query, anchor) becomes
 *   d_loops[m] = (query, anchor, shift, dist) and suppresses every pair with |q' - q| <= spread and |a' - a| <= spread; a round without a
 *   pair writes (-1, -1, 0, 0).  n_loops is the number of rounds filled.  d_rep = (n_pairs, n_known, n_loops, 0).
 * Three launches: the closure edges compacted (one workgroup), one lane per record against them (known or not), the rounds in one
 * workgroup -- keys of distinct integers, so no reduction order matters.  d_workspace: lsd_pg_loops_workspace_bytes(n_q, k, edges_cap)
 * bytes of the caller's, 8-byte aligned, their contents unspecified (0 for arguments this entry refuses).  n_q == 0 is "no pair".
 * LSD_ERR_INVALID before anything is enqueued, outputs untouched: a null pointer; nodes_cap outside 1..16384, edges_cap outside
 * 1..65536; max_loops outside 1..LSD_PG_LOOPS_MAX; spread < 0; k outside 1..LSD_PG_PLACE_MAX; q_lo < 0, n_q < 0 or q_lo + n_q >
 * nodes_cap; a pointer not 8-byte aligned. */
typedef struct lsd_pg_loops_par { int32_t max_loops, spread; } lsd_pg_loops_par;                          /* 8 bytes */
typedef struct lsd_pg_loop_rec  { int32_t query, anchor, shift; uint32_t dist; } lsd_pg_loop_rec;          /* 16 bytes */
typedef struct lsd_pg_loops_rep { int32_t n_pairs, n_known, n_loops, reserved; } lsd_pg_loops_rep;         /* 16 bytes */
#define LSD_PG_LOOPS_MAX 64
size_t lsd_pg_loops_workspace_bytes(int n_q, int k, int edges_cap);
int lsd_enqueue_pg_loops_device(lsd_ctx *ctx, const lsd_pg_place_rec *d_recs, const lsd_pg_place_rep *d_reps, int q_lo, int n_q, int k,
                                const lsd_pg_head *d_head, int nodes_cap, const lsd_pg_edge *d_edges, int edges_cap, lsd_pg_loops_par par,
                                void *d_workspace, lsd_pg_loop_rec *d_loops /* par.max_loops */, lsd_pg_loops_rep *d_rep, void *stream);
/* lsd_enqueue_pg_loop_select_device: what lsd_enqueue_pg_recognize_device leaves, for loop m.  With L = d_loops[m] (d_loops holds at least
 * m + 1 records) the outputs d_near, d_sel, d_q_scan, d_q_len and d_q_pose are written exactly as that entry writes them for the anchor
 * L.anchor, shift L.shift, dist L.dist and the query j = L.query: d_near = (anchor, j, n_cand = d_loops_rep->n_loops, 0, d2 = (double)dist);
 * d_sel[k] = node k's pose iff |k - anchor| <= window and k <= j - gap, else the sentinel; the gathered row is store row j with its
 * length; d_q_pose = (x_A, y_A, wrap(ang_A - shift * 5.625)).  An unfilled m (query == -1) gives that entry's "no query" outputs: anchor
 * -1, d_q_len = 0, the sentinel pose, the row keeps its bytes, d_sel all sentinels.  (A query outside 0..N-1 reads as no query and an anchor
 * outside 0..N-1 as no anchor: records that no batch left.)  lsd_enqueue_pg_closure_device takes the query from the near record, so the
 * chain behind lsd_enqueue_pg_near_device runs on these outputs unchanged.  One launch of one workgroup.  LSD_ERR_INVALID before anything
 * is enqueued, outputs untouched: a null pointer; nodes_cap outside 1..16384; store_stride outside 1..the context's scan capacity; gap < 1
 * or window < 0; m outside 0..LSD_PG_LOOPS_MAX-1; the alignments of lsd_enqueue_pg_near_device, d_loops and d_loops_rep 8-byte. */
int lsd_enqueue_pg_loop_select_device(lsd_ctx *ctx, const lsd_pg_head *d_head, const lsd_pg_node *d_nodes, int nodes_cap,
                                      const lsd_polar *d_store, const int *d_store_lens, int store_stride, int gap, int window,
                                      const lsd_pg_loop_rec *d_loops, const lsd_pg_loops_rep *d_loops_rep, int m, lsd_pg_near_rec *d_near,
                                      lsd_position *d_sel, lsd_polar *d_q_scan, int *d_q_len, lsd_position *d_q_pose, void *stream);
/* lsd_enqueue_pg_reduce_device: keyframes that add nothing are taken out, the odometry chain is contracted across them, and nodes, edges,
 * tracks, store rows, lengths and descriptors are compacted in place, so that a graph that patrols the same places stops growing
 * (csrc/k_pgreduce.hip; restated in tests/pose_graph_reduce_cases.py).  d_tracks: ALL n_tracks track records of the graph;
 * d_desc: the descriptors of lsd_enqueue_pg_describe_device, or NULL for a graph that keeps none.  N and E are the clamped counts.  fp64
 * without FMA; every sum runs ascending from 0.0; SKIPPED is the relaxation's definition above, W the symmetric matrix of an edge's info.
 *   CELL.  A node whose x, y and ang are finite has the cell (floor(x / cell), floor(y / cell), floor(wrap(ang) / ang_bin)).  The three
 *   components are kept as the fp64 values floor returns -- integers of any size, or an infinity where the quotient overflows -- and two
 *   cells are the same where all three compare == : there is no integer type whose range could be left.  Any other node has no cell.
 *   rank(k) = the number of nodes i < k that have k's cell (a count: no order).  REDUNDANT: k has a cell and rank(k) >= keep.
 *   REMOVABLE: k is not LSD_PG_NODE_FIXED; no track record has last == k; among the edges that are not skipped exactly two touch k, one
 *   with j == k (its INCOMING edge) and one with i == k (its OUTGOING edge); both have LSD_PG_EDGE_CLOSURE clear; inv3(W) of both succeeds.
 *   MARKED: redundant and removable.  (Degrees and edge ids come from integer sums and minima.)
 *   RUNS.  An edge e = (a, r) that is not skipped, with a not marked and r marked, HEADS a run.  z = e.z, S = inv3(W_e), len = 1, cur = r.
 *   A step: with f = (cur, b) the outgoing edge of cur, zn = f.z, Sn = inv3(W_f), (s, c)(z.ang), k = pi / 180.0,
 *     J1 = [(1.0, 0.0, k * ((-s) * zn.x - c * zn.y)), (0.0, 1.0, k * (c * zn.x - s * zn.y)), (0.0, 0.0, 1.0)]
 *     J2 = [(c, -s, 0.0), (s, c, 0.0), (0.0, 0.0, 1.0)]
 *     T(r,q) = sum_t J1(r,t) * S(t,q), U1(r,q) = sum_t T(r,t) * J1(q,t);  T'(r,q) = sum_t J2(r,t) * Sn(t,q), U2(r,q) = sum_t T'(r,t) * J2(q,t)
 *     S = U1 + U2 (all nine elements, every product made, the zeros' too);  then z = comp(z, zn)
 *   b not marked: the run ends at b.  b marked and len == max_run: b is UN-MARKED, the run ends at b, and where the outgoing edge of b leads
 *   to a marked node that edge heads the next run, walked by the same owner.  Otherwise cur = b, len += 1, the next step.
 *   A run is CONTRACTED when b != a, z[3] and S[9] are finite and I = inv3(S) succeeds: its len nodes are RETIRED, the slot of the heading
 *   edge receives (i = a, j = b, flags = LSD_PG_EDGE_CONTRACTED, reserved = 0, z, info = I(0,0), I(0,1), I(1,1), I(0,2), I(1,2), I(2,2), chi2 =
 *   +0.0) and the outgoing edges of its len nodes are dropped.  Any other run is KEPT WHOLE: nothing of it changes.  A marked node that no
 *   run reached (a ring without an unmarked node) stays as well.
 *   EDGES.  An edge with both ends in 0..N-1 and a retired end that is neither heading nor part of a contracted run (only a skipped edge
 *   can be one) is dropped and counted.  The surviving edges keep their relative order; one with both ends in 0..N-1 has them renumbered,
 *   one with an end outside keeps all its bytes.
 *   COMPACTION.  d_map[k] = the new index of node k, k < N; -1 for a retired one and for N <= k < nodes_cap.  The surviving node records
 *   (64 bytes), store rows (store_stride readings), lengths and descriptors (72 bytes) are at their new index, the order kept; a track's
 *   last in 0..N-1 is renumbered, every other byte of a track kept; the head has the new counts.  From the new n_nodes up to N the
 *   lengths are 0 -- empty scans to the integration -- and the descriptors all zero -- "not described", so that
 *   lsd_enqueue_pg_describe_device describes what is appended there next --; node records and store rows there, and the edge records
 *   from the new n_edges on, keep the bytes they had when the call began.
 *   REPORT: nodes and edges before and after; nodes redundant, marked, retired; runs contracted and kept whole; the most nodes of one
 *   contracted run; edges dropped for a retired end; flags: RETIRED iff a node was retired, SPLIT iff max_run ended a run.
 *   A call that reports no SPLIT is idempotent: the same call again changes no byte but rewrites the map and the report.  A call that
 *   reports SPLIT is NOT: a node that max_run un-marked is still redundant and removable, so the next call retires it (it and no other
 *   node), and repeated calls end at a graph that no further call changes.
 * A fixed number of launches on `stream` that depends on nodes_cap alone (8 + 1 + ceil(nodes_cap / 1024)); no workgroup waits for
 * another, every loop is bounded by N, E or a parameter (a walk visits no node twice: a marked node has one incoming edge that counts,
 * and the walk began at an unmarked node, so it cannot come back into what it has walked), no atomics on fp64, no allocation, no host wait.  LSD_ERR_INVALID before anything
 * is enqueued, outputs untouched: a null pointer (d_desc and d_rep may be NULL); nodes_cap outside 1..16384, edges_cap outside 1..65536;
 * store_stride outside 1..the context's scan capacity; n_tracks < 1; cell or ang_bin not finite or <= 0, ang_bin > 360; keep < 1, max_run
 * < 1; store or workspace not 16-byte, a record array, the descriptors or d_rep not 8-byte, lengths or d_map not 4-byte aligned.
 * lsd_pg_reduce_workspace_bytes: 0 for arguments outside those limits (a store_stride < 1 is one). */
typedef struct lsd_pg_reduce_par { double cell, ang_bin; int32_t keep, max_run; } lsd_pg_reduce_par;    /* 24 bytes */
typedef struct lsd_pg_reduce_rep {         /* 48 bytes */
    int32_t nodes_before, edges_before, nodes_after, edges_after, redundant, marked, retired, runs, runs_kept, longest_run, dropped_edges;
    uint32_t flags;
} lsd_pg_reduce_rep;
#define LSD_PG_EDGE_CONTRACTED 8u
#define LSD_PG_REDUCE_RETIRED 1u
#define LSD_PG_REDUCE_SPLIT 2u
size_t lsd_pg_reduce_workspace_bytes(int nodes_cap, int edges_cap, int store_stride);
int lsd_enqueue_pg_reduce_device(lsd_ctx *ctx, lsd_pg_head *d_head, lsd_pg_node *d_nodes, int nodes_cap, lsd_pg_edge *d_edges, int edges_cap,
                                 lsd_pg_track *d_tracks, int n_tracks, lsd_polar *d_store, int *d_store_lens, int store_stride,
                                 lsd_pg_desc *d_desc /* may be NULL */, lsd_pg_reduce_par par, int32_t *d_map /* nodes_cap */,
                                 lsd_pg_reduce_rep *d_rep /* may be NULL */, void *d_workspace, void *stream);
/* Host conveniences: host arrays of any alignment, staged through the context; blocking.
 * lsd_pg_reduce: the graph (head, nodes[nodes_cap], edges[edges_cap], tracks[n_tracks], store, store_lens, desc[nodes_cap] or NULL) makes
 * the round trip around lsd_enqueue_pg_reduce_device; map[nodes_cap] and rep receive the map and the report.
 * lsd_pg_describe: n scans (scans[n * stride], lens[n]) -> desc_out[n], every row described; n outside 0..16384: LSD_ERR_INVALID.
 * lsd_pg_recognize: desc[n_nodes] and a query index -> recs[par.k] and rep; no selection and no gather are written, par.window is
 * checked and not used; n_nodes outside 1..16384: LSD_ERR_INVALID.
 * lsd_pg_recognize_all: desc[n_nodes] and the queries q_lo .. q_lo + n_q - 1 -> recs[n_q * par.k] and reps[n_q], around
 * lsd_enqueue_pg_recognize_all_device with nodes_cap = n_nodes; n_nodes outside 1..16384: LSD_ERR_INVALID; n_q == 0 writes nothing.
 * lsd_pg_loops: recs[n_q * k], reps[n_q] and the graph's edges[n_edges] -> loops[par.max_loops] and rep, around
 * lsd_enqueue_pg_loops_device; n_q outside 0..16384 or n_edges outside 0..65536: LSD_ERR_INVALID.
 * lsd_pg_relax: one graph; nodes[n_nodes] and edges[n_edges] are updated in place, rep receives the report.
 * lsd_pg_relax_robust: the same around lsd_enqueue_pg_relax_robust_device; rep and rob_rep receive the two reports.
 * lsd_pg_relax_pc: the same around lsd_enqueue_pg_relax_pc_device; rep, rob_rep and pc_rep receive the three reports.
 * lsd_pg_append: the graph (head, nodes[nodes_cap], edges[edges_cap], track, store, store_lens) makes the round trip around the device
 * entry with the n_cand candidates; lens[t] outside 0..stride: LSD_ERR_INVALID. */
int lsd_pg_relax(lsd_ctx *ctx, lsd_pg_node *nodes, int n_nodes, lsd_pg_edge *edges, int n_edges, lsd_pg_relax_par par,
                 lsd_pg_relax_rep *rep);
/* lsd_pg_marginals: one graph (nodes[n_nodes], edges[n_edges], neither changed) and queries[n_q] -> recs[n_q] and rep, around
 * lsd_enqueue_pg_marginals_device; prior_edges < 0: no prior, else a prior head whose n_edges is prior_edges.
 * lsd_pg_vet: the graph, queries[n_q] and recs[n_q] -> the edges' flags in place and reps[n_q] (may be NULL), around
 * lsd_enqueue_pg_vet_device. */
int lsd_pg_marginals(lsd_ctx *ctx, const lsd_pg_node *nodes, int n_nodes, const lsd_pg_edge *edges, int n_edges, int prior_edges,
                     const lsd_pg_marg_query *queries, int n_q, lsd_pg_marg_par par, lsd_pg_marg_rec *recs, lsd_pg_marg_rep *rep);
int lsd_pg_vet(lsd_ctx *ctx, const lsd_pg_node *nodes, int n_nodes, lsd_pg_edge *edges, int n_edges, const lsd_pg_marg_query *queries,
               const lsd_pg_marg_rec *recs, int n_q, double gate, lsd_pg_vet_rep *reps);
int lsd_pg_relax_robust(lsd_ctx *ctx, lsd_pg_node *nodes, int n_nodes, lsd_pg_edge *edges, int n_edges, lsd_pg_relax_par par,
                        lsd_pg_robust_par rob, lsd_pg_relax_rep *rep, lsd_pg_robust_rep *rob_rep);
int lsd_pg_relax_pc(lsd_ctx *ctx, lsd_pg_node *nodes, int n_nodes, lsd_pg_edge *edges, int n_edges, lsd_pg_relax_par par,
                    lsd_pg_robust_par rob, lsd_pg_precond_par pc, lsd_pg_relax_rep *rep, lsd_pg_robust_rep *rob_rep,
                    lsd_pg_precond_rep *pc_rep);
int lsd_pg_append(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n_cand, int stride, const lsd_position *poses,
                  lsd_pg_head *head, lsd_pg_node *nodes, int nodes_cap, lsd_pg_edge *edges, int edges_cap, lsd_pg_track *track_rec,
                  int32_t track, lsd_polar *store, int *store_lens, int store_stride, lsd_pg_append_par par, lsd_pg_append_rep *rep);
int lsd_pg_describe(lsd_ctx *ctx, const lsd_polar *scans, const int *lens, int n, int stride, double range_max, lsd_pg_desc *desc_out);
int lsd_pg_recognize(lsd_ctx *ctx, const lsd_pg_desc *desc, int n_nodes, int query, lsd_pg_place_par par, lsd_pg_place_rec *recs,
                     lsd_pg_place_rep *rep);
int lsd_pg_recognize_all(lsd_ctx *ctx, const lsd_pg_desc *desc, int n_nodes, int q_lo, int n_q, lsd_pg_place_par par,
                         lsd_pg_place_rec *recs, lsd_pg_place_rep *reps);
int lsd_pg_loops(lsd_ctx *ctx, const lsd_pg_place_rec *recs, const lsd_pg_place_rep *reps, int n_q, int k, const lsd_pg_edge *edges,
                 int n_edges, lsd_pg_loops_par par, lsd_pg_loop_rec *loops, lsd_pg_loops_rep *rep);
int lsd_pg_reduce(lsd_ctx *ctx, lsd_pg_head *head, lsd_pg_node *nodes, int nodes_cap, lsd_pg_edge *edges, int edges_cap, lsd_pg_track *tracks,
                  int n_tracks, lsd_polar *store, int *store_lens, int store_stride, lsd_pg_desc *desc /* may be NULL */,
                  lsd_pg_reduce_par par, int32_t *map, lsd_pg_reduce_rep *rep);

/* --- introspection used by the parity tests and the bench ------------------------------- */
/* Scaled size of a cols x rows map: w = floor(cols*sca), h = floor(rows*sca) (myLSD.cpp:132-133). */
void lsd_scaled_size(int cols, int rows, double sca, int *w, int *h);

/* Stops the pipeline after a stage (parity tests of intermediate maps); 0 = run everything. */
enum { LSD_STAGE_ALL = 0, LSD_STAGE_GAUSS = 1, LSD_STAGE_GRAD = 2, LSD_STAGE_SORT = 3, LSD_STAGE_REGION = 4 };
int lsd_set_stop_after(lsd_ctx *ctx, int stage);
/* Enables the per-seed trace buffer (LSD_DBG_SEEDS); costs one record store per grown seed. */
int lsd_set_trace(lsd_ctx *ctx, int on);
/* The fused front end (default 1): for the reference's 17 Gaussian taps (sca 0.3, sig 0.6) the Gaussian and the gradient pass run as
 * one kernel and GaussImage never exists in device memory; 0 runs them as two kernels with the image in between, as every other tap
 * count, lsd_set_stop_after(LSD_STAGE_GAUSS) and lsd_set_trace do anyway.  Results are identical.  On the fused path lsd_last_timings
 * reports the kernel under "gauss" and "gradient" as exactly 0, the per-image Gaussian workspace (8 B per scaled pixel) is not
 * allocated, and LSD_DBG_GAUSS is recomputed on demand (lsd_debug_fetch). */
int lsd_set_fused_front(lsd_ctx *ctx, int on);
/* Lines in the region stage (default 1): the region stage's workgroup writes the line records and the lineIm marks of an image when it
 * has finished that image, instead of a kernel behind the whole batch -- one kernel launch less per call, and an image's lines do not
 * wait for the slowest image.  0 runs that kernel, as lsd_set_trace and lsd_set_region_help do anyway.  Results are identical.  On the
 * fused path lsd_last_timings reports "lines" as exactly 0 (the work is under "region"). */
int lsd_set_fused_lines(lsd_ctx *ctx, int on);
/* Region stage variant: 4 wavefronts per image (three images per CU: the throughput build) or 8 (one image per CU, ~1.5x lower
 * latency per image, images taken heaviest first).  0 (default) picks 8 while the batch has at most four images per CU (the step is
 * bounded by its heaviest image until then) and 4 beyond.  Results do not depend on the choice.  Set it before lsd_reserve: the
 * per-wave workspace (8 B per scaled pixel and wavefront + result slots) is sized for the variant. */
int lsd_set_region_waves(lsd_ctx *ctx, int waves);
/* Help across workgroups in the region stage: wavefronts of workgroups whose image is finished evaluate seeds of the images still
 * running (up to `waves` helper wavefronts per image; 0 or -1, the default since round 6: none); an image asks once it has run for
 * ~5 ms with its own wavefronts busy, and a call with up to four images also gets helper-only workgroups from the start.  OFF by
 * default: it paid while single images were dominated by long uniform structures grown again and again (round 4: a heavy 2048 x 2048
 * map 77 -> 30 ms); since those are answered from certified sets it ties or loses at every call size (one heavy map 50.5 ms with, 49.9
 * without; two 59.2 / 49.7; 64 maps 51.4 / 50.2; 512 maps 83 / 78; the reference's maps one per call 1.01 / 0.96 ... 6.37 / 6.36 ms:
 * profiles/r06q_help_small_probe.log), and a caller that keeps several batches in flight needs none either.  The machinery stays
 * available and tested (lsd_set_region_help(ctx, 24)); results do not depend on it. */
int lsd_set_region_help(lsd_ctx *ctx, int waves);
/* Scheduling hint: "the batches this context gets hold the same maps from call to call" (a site's maps, re-extracted as they are
 * updated).  The region stage then starts the images in descending order of the time each one took in the context's previous call with
 * the same number of images, instead of by their count of gradient pixels (which predicts the cost poorly): a batch run alone ends with
 * its heaviest image, and that image should start first.  Off by default; results never depend on it. */
int lsd_set_cost_history(lsd_ctx *ctx, int on);
/* Test hook: the region stage marks the pixels of the region it is growing with a fresh 32-bit id per grow; a wavefront that
 * uses up its 2^20 ids within one run clears its stamp array and starts over.  That takes more than a million grows by one
 * wavefront on one image; this lowers the budget (2 .. 0xFFFF0 grows) so that tests reach the path.  Results do not change. */
int lsd_debug_set_stamp_budget(lsd_ctx *ctx, unsigned grows);
/* Test / developer hook: a schedule setting of the region stage by name ("SOFT", "CLAIM", "FEED", "BIG", "EARLY", "WB", "GATE", "SHARE",
 * "UP", "DOWN", "REQUEUE", "XPOLL", "LINGER", "HELP", "POOL"; csrc/lsd_ctx.hip: kTunings), clamped to its range, or "FA_LDS": the number
 * of kept candidates up to which FeatureAssociation sorts in LDS (0..1024, default 1024; beyond it, in global memory).  None changes a
 * result.  From the ENVIRONMENT the shipped library takes two settings only, when a context is created: LSD_REGION_HELP (as
 * lsd_set_region_help) and LSD_REGION_POOL (calls with at most that many images, 0..16, default 4, get helper-only workgroups). */
int lsd_debug_set_tuning(lsd_ctx *ctx, const char *name, int value);
/* Test hook: fills the workspace arrays that the front end writes (GaussImage, magMap, degMap, the (sin, cos) table, the packed pixel
 * words, the sorted lists and their lengths) with 0xFF bytes over their whole capacity (synchronises).  The next call has to store
 * every value itself: without this a store it leaves out hides behind what the previous call left at the same address.  Call it
 * after a call of the same shape and batch size, so that the workspace is already the size the next call needs. */
int lsd_debug_poison_front(lsd_ctx *ctx);

/* Copies an intermediate of image `image` of the LAST run/enqueue to host memory (synchronises).
 *   GAUSS/MAG/DEG  h*w doubles      (GaussImage / magMap / degMap, myLSD.cpp:143-147)
 *   STATE          h*w uint32       usedMap value 0 / 1 / 2 (myLSD.cpp:145)
 *   ORDER          nb uint32        sorted seed list, element = y*w + x (binCell after qsort, :204)
 *   ORDER_VAL      nb uint16        its bin values
 *   NB             1 int32          len_binCell
 *   MAXGRAD        1 double
 *   RECS           count*12 doubles accepted structRec before rescale (x1 y1 x2 y2 wid cX cY deg dx dy p prec)
 *   SEEDS          n_seed records {int order_idx, x, y, num, outcome, final_num; double logNFA}
 *   NSEED          1 int32
 *   STATS          32 int64         grow_calls, grown_px, nfa_calls, rrr_calls, rrr_passes, rrr_sentinel, rrr_oob, cycles_rrr*,
 *                                   cycles_total, cycles_grow*, cycles_rect*, cycles_nfa*, cycles_mark*, max_region*, nfa_px*, seeds,
 *                                   exact_angle_evals*, tile_fetches*, batches*, cycles_tiles*, spec_redos, spec_discards, cycles_wait*,
 *                                   resweep_batches*, slow_batches*, cycles_eval*, cycles_sums*, cycles_refine*, cycles_idle*,
 *                                   cycles_select*, cycles_commit*, filter_skips*
 *                                   (summed over the wavefronts that share an image; * = counted by the developer build only,
 *                                   `make stats` -> liblsdhip_stats.so, and 0 in the product build).  Word 45 of the record (48 words
 *                                   are kept per image): bits 3..0 the XCC the image ran on, bits 8.. the RegionGrower calls that took
 *                                   the any-tolerance function (tolerances of 1.5 rad and more, NaN: csrc/region/grow.h, grow_any())
 *   SINCOS         h*w*2 doubles    (sin, cos) of degMap as the gradient pass leaves them for RegionGrower (myLSD.cpp:545-546), one pair
 *                                   per pixel.  Entries are DEFINED ONLY WHERE THE PIXEL'S CODE IS 0 after the gradient pass (PW & 3,
 *                                   == usedMap before the region stage): (0, 1) on row 0 / column 0 (an interior pixel without
 *                                   gradient has code 1 whenever gradThre > 0); every other entry is whatever an earlier call left there
 *   PW             h*w uint32       the packed pixel word itself, the only thing RegionGrower reads per neighbour: the fp32 angle
 *                                   with its two lowest mantissa bits replaced by the code 0 free / 1 banned by the gradient threshold
 *                                   / 2 marked by a rejected region / 3 banned by an accepted line (STATE is this word reduced to usedMap)
 *   GRAD_TIES      1 int32          the gradient pass's share of lsd_last_sensitivity (which also needs the region stage to have run)
 * After a call that took the fused front end (lsd_set_fused_front) there is no GaussImage to copy: GAUSS runs the Gaussian kernel alone
 * on the requested image of the last call's INPUT, so for lsd_enqueue_batch_device the caller's d_maps must still be alive and
 * unchanged when GAUSS is fetched (a map the call itself rewrote, LSD_FLAG_WRITEBACK_MAP, is read as rewritten; the host entry points
 * keep their own copy).
 * Returns LSD_ERR_INVALID if `bytes` is smaller than the item. */
enum { LSD_DBG_GAUSS = 1, LSD_DBG_MAG, LSD_DBG_DEG, LSD_DBG_STATE, LSD_DBG_ORDER, LSD_DBG_ORDER_VAL,
       LSD_DBG_NB, LSD_DBG_MAXGRAD, LSD_DBG_RECS, LSD_DBG_SEEDS, LSD_DBG_NSEED, LSD_DBG_STATS,
       LSD_DBG_SINCOS, LSD_DBG_PW, LSD_DBG_GRAD_TIES };
int lsd_debug_fetch(lsd_ctx *ctx, int image, int what, void *out, size_t bytes);

/* Test hook: evaluates the DEVICE build of the path's transcendental functions on host arrays of n
 * doubles: fn 0 = sin/cos(a) -> out0,out1; fn 1 = atan2(a, b) -> out0; fn 2 = atan(a) -> out0;
 * fn 3 = the region stage's fp32 ESTIMATE of sin/cos of the packed angle of a (its error bound is a test). */
int lsd_debug_eval_math(lsd_ctx *ctx, int fn, const double *a, const double *b, double *out0, double *out1, size_t n);

/* Test hook: K5 alone (csrc/k_lines.hip) on n caller-given rectangles recs[n][4] = x1 y1 x2 y2, already in the map's cells, as one
 * image of cols x rows: lines_out[n] receives the records (bytes K5 does not write stay 0xFF) and line_im, rows x cols or NULL,
 * the raster.  End points no map produces -- a sample exactly half-way between two cells, x1 == x2 and y1 == y2 -- reach K5 only
 * through here.  Keep |coordinates| small: the walk visits every integer between the end points. */
int lsd_debug_lines(lsd_ctx *ctx, const double *recs, int n, int cols, int rows, lsd_line *lines_out, uint8_t *line_im);

/* Profiling hook: streams `bytes` once with 8-B-per-lane stores (k_calib_write8) and once with 8-B-per-lane loads
 * (k_calib_read8) so that rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE can be calibrated for the front end's access shape. */
int lsd_debug_calibrate(lsd_ctx *ctx, size_t bytes);

/* Per-kernel device time (ms) of the last lsd_run/lsd_run_batch, measured with HIP events on the
 * context's stream: [0] gauss, [1] gradient, [2] sort, [3] region, [4] lines, [5] total. */
int lsd_last_timings(lsd_ctx *ctx, float ms_out[6]);

#ifdef __cplusplus
}
#endif
#endif /* LSD_HIP_H */
