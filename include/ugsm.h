/*
 * ugsm.h -- C-ABI of libugsm.so: the MI355X (gfx950) pyramidal dense stereo matcher
 * that replaces ug_stereomatcher's MatchGPULib + MatchLib.cu behind the
 * UG_matcher_gpu node / GetDisparitiesGPU.srv.
 *
 * Plain C, plain pointers and sizes; no torch, OpenCV or ROS types.  File:line
 * citations are relative to /root/reference/src/gpu_matcher/ and name the reference
 * interface each entry point replaces.  The reference's own C boundary
 * (25 one-kernel `extern "C"` wrappers, MatchLib_common.h:35-74 and
 * MatchGPULib.cpp:45-247) is deliberately NOT replicated: that granularity is what
 * forces ~130 launches per iteration.  INTEGRATION.md shows the MatchGPULib shim and
 * the node-side binding.
 *
 * Threading: calls on one ctx must be serialised by the caller (the reference node
 * is a single-threaded ros::spin, UG_GPU_matcher.cpp:749-752).  Different slots of a
 * ctx run concurrently on the device.  No entry point calls exit(); every failure is
 * a status code (reference: checkCudaErrors -> exit(EXIT_FAILURE)).
 */
#ifndef UGSM_H
#define UGSM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libugsm.so is built with -fvisibility=hidden: what this header declares is everything the library exports (nm -D lists ugsm_* only). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define UGSM_ABI_VERSION 6  /* 6 (additions, nothing changed): the coloured point cloud -- ugsm_cloud_params, UGSM_CLOUD_PCL32 / UGSM_CLOUD_XYZRGB16,
                               ugsm_default_cloud_params, ugsm_cloud_points, ugsm_point_cloud, ugsm_point_cloud_fovea; the resized cloud --
                               ugsm_resized_cloud_points, ugsm_point_cloud_resized, ugsm_point_cloud_resized_fovea; the input formats --
                               UGSM_INPUT_*, ugsm_input_bytes_per_pixel, ugsm_input_format_from_encoding, ugsm_set_input_format,
                               ugsm_get_input_format; the merged cloud of the fovea stack -- ugsm_fovea_level_mapping, ugsm_fovea_cloud_points,
                               ugsm_point_cloud_fovea_all; the LR check of the foveated calls -- UGSM_LR_FULL / UGSM_LR_FOVEATED, ugsm_set_lr_check,
                               ugsm_get_lr_check, ugsm_last_lr_marked_levels; the merged cloud of several windows' stacks --
                               ugsm_fovea_multi_cloud_points, ugsm_point_cloud_fovea_multi; the warped right image and the photometric residual of a
                               match -- ugsm_warp_planes, ugsm_warp_right, ugsm_warp_right_fovea, ugsm_photometric_residual,
                               ugsm_photometric_residual_fovea; the checked full-mode call -- ugsm_submit_full_checked, ugsm_match_full_checked,
                               ugsm_last_lr_marked_pair; the seeded full-mode call -- ugsm_submit_full_seeded, ugsm_match_full_seeded,
                               ugsm_stage_restrict, ugsm_seeded_pixel_iterations; the seeded (warm) foveated call -- ugsm_submit_foveated_warm,
                               ugsm_submit_foveated_warm_field, ugsm_match_foveated_warm, ugsm_stage_warm_stack, ugsm_fovea_warm_pixel_iterations;
                               the full-mode call in two halves -- ugsm_submit_full_coarse, ugsm_submit_full_fine, ugsm_match_full_coarse,
                               ugsm_match_full_fine, ugsm_stage_prolong, ugsm_coarse_pixel_iterations; checked full-mode pairs through the queue --
                               ugsm_submit_full_checked_host, ugsm_enqueue_full_checked, ugsm_enqueue_full_checked_managed,
                               ugsm_enqueue_full_checked_cloud, ugsm_enqueue_full_checked_cloud_managed, ugsm_checked_result, ugsm_done_checked;
                               the depth image (REP 118 32FC1 / 16UC1) -- ugsm_depth_params, UGSM_DEPTH_32F / UGSM_DEPTH_16U / UGSM_DEPTH_ALL_LEVELS,
                               ugsm_default_depth_params, ugsm_depth_image_size, ugsm_depth_image, ugsm_depth_image_fovea, ugsm_match_full_depth,
                               ugsm_depth_image_fovea_full, ugsm_depth_image_fovea_multi, ugsm_match_foveated_depth;
                               lens distortion in triangulation, clouds and depth -- ugsm_set_lens, ugsm_get_lens, ugsm_undistort_points
                               6: the kernel choices follow what is in flight, not ugsm_config.slots: ugsm_plan_level takes `alone`, ugsm_plan_level_in_frame
                               is gone, ugsm_level_plan.latency_policy is .alone; ugsm_enqueue_* returns UGSM_OK once the pair is accepted (a failed
                               CALL is reported through ugsm_completion.status only); the fovea shard carries a status word (a rank that fails still
                               reaches the exchange); march_min_pixels < 0 and march_smooth are libugsm_dev.so's
                               5: the queue (ugsm_enqueue_*, ugsm_flush, ugsm_next_done, ugsm_queue_depth, ugsm_queue_plan, ugsm_poll; UGSM_PENDING / UGSM_EMPTY),
                               RCCL inside the library (ugsm_shard_*), hidden visibility for everything else
                               4: ugsm_config grew (batch, stream_priority), ugsm_submit_full_batch, ugsm_submit_foveated_batch; kernel_path 1,
                               march_smooth and the probe entry points moved to libugsm_dev.so (include/ugsm_dev.h)
                               3: ugsm_config grew (lr_check_threshold, streams), ugsm_stage_lr_check, ugsm_slot_stream, ugsm_last_lr_marked,
                               ugsm_submit_full_host, ugsm_submit_foveated_host, ugsm_plan_level_in_frame */

/* status codes */
#define UGSM_OK                0
#define UGSM_ERR_BAD_ARG       1  /* null pointer, non-positive size, bad slot/level, image above 2^28 pixels */
#define UGSM_ERR_SIZE_MISMATCH 2  /* left/right differ, or stride < bytes per pixel * W (ref: unchecked, MatchGPULib.cpp:315-323) */
#define UGSM_ERR_TOO_SMALL     3  /* a pyramid level would be < 1 px (ref: zero-size malloc, MatchGPULib.cpp:1247) */
#define UGSM_ERR_NO_DEVICE     4  /* no HIP device / HIP runtime unusable */
#define UGSM_ERR_DEVICE        5  /* a HIP call failed; see ugsm_last_error */
#define UGSM_ERR_NOMEM         6
#define UGSM_ERR_STATE         7  /* e.g. fine phase without coarse phase */
#define UGSM_PENDING           8  /* not an error: ugsm_poll / ugsm_next_done(block = 0) -- the work asked about has not finished yet */
#define UGSM_EMPTY             9  /* not an error: ugsm_next_done -- every pair enqueued so far has been reported */
#define UGSM_ERR_PEER          10 /* the fovea shard: another rank failed its part of the step (this rank's result is not valid), or no rank answered
                                     within the deadline and the communicator was aborted; ugsm_last_error says which */

#define UGSM_MAX_LEVELS 32
#define UGSM_MAX_BATCH 16  /* pairs per ugsm_submit_*_batch call */

typedef struct ugsm_ctx ugsm_ctx;

/* Replaces the compile-time/argv configuration of the reference:
 *   device        <- "-device=N" parsed by findCudaDevice, MatchGPULib.cpp:254
 *   levels        <- MAX_LEVEL, MatchLib_common.h:13 (14)
 *   fovea_levels  <- foveatelevel = argv[2] or 7, MatchGPULib.cpp:259-264
 *   slots         <- pairs in flight (one HIP stream each); the reference has 1
 *   kernel_path   <- 0: fused gfx950 kernels (default, and the only path of libugsm.so); 1: one-stage-per-kernel
 *                    path kept for A/B parity checks (same results bit for bit) -- in libugsm_dev.so only since ABI 4,
 *                    libugsm.so answers UGSM_ERR_BAD_ARG
 *   march_*       <- which levels run the marching form of the cost kernel (same results bit for bit) */
typedef struct ugsm_config {
    int device;
    int levels;
    int fovea_levels;
    int slots;
    int kernel_path;
    int profile_events; /* slot 0 times its launches with HIP events carried in the dispatch (the kernel's own begin and end): 1 = the cost kernel only, 2 = every kernel class */
    int march_min_pixels; /* at least this many pixels march; levels no other form covers march too.  K-cost as the marching
                             kernel (one wave per strip of columns, no LDS) for the levels of at least this many pixels per launch,
                             and for every level that neither k_cost_march4 nor the coarse-level latency form takes (with this
                             threshold above k_cost_march4's 3 Mpx, say); 0 = default threshold (0.4 Mpx per launch; in effect 3 Mpx:
                             the channel-parallel form k_cost_march4 takes the levels below first); < 0 = never: round 1's LDS-tiled
                             k_cost_split takes the levels no other form covers -- libugsm_dev.so only since ABI 6 (libugsm.so
                             answers UGSM_ERR_BAD_ARG) */
    int march_np;         /* ignored since ABI 3 (kept for layout): the two-pixels-per-lane development form of the marching kernel
                             is no longer in the library (tools/kbench.hip instantiates it) */
    int march_rows;       /* tuning / tests: strip height of the marching kernel (0 = automatic) */
    int march_smooth;     /* ignored since ABI 6 (kept for layout): the marching K-smooth, bit-identical and measured slower than the
                             LDS-tiled one (docs/HISTORY.md), is no longer built */
    float early_exit_threshold; /* SURVEY 8f row f-4, OFF at 0 (default): when > 0, a level stops iterating as soon as the
                             confidence-weighted mean change of dx and of dy between two iterations is below it
                             (differenceIterations / weightedDifference, MatchGPULib.cpp:1323-1437 -- dead code in the
                             reference, whose results this option therefore leaves; one host round trip per iteration) */
    int small_max_pixels; /* levels of at most this many pixels run K-cost / K-smooth in their latency forms (ugsm_kernels_small.hip:
                             channel-parallel 16 x 12 tiles, one thread per pixel; same results bit for bit); 0 = default
                             threshold (0.15 Mpx for a call that has the chip to itself, 50 k pixels for one that shares it), < 0 = never */
    float lr_check_threshold; /* LR-consistency check, OFF at 0 (default).  Named by the north star; THE REFERENCE HAS NONE (no
                             right-to-left pass in MatchLib.cu / MatchGPULib.cpp), so any value > 0 leaves the reference's results:
                             full mode only (ugsm_match_full / ugsm_submit_full), the pair is matched a second time with the images
                             exchanged, and the confidence of every left pixel whose match (x + dx, y + dy) in the right-to-left
                             field does not point back within this many pixels, in x or in y, is set to 0 (dx, dy unchanged).
                             Doubles the matching work of a call.  The foveated calls take the check through ugsm_set_lr_check
                             (below), which also changes or switches off the threshold of a live context. */
    int streams;          /* HIP streams the slots' work is dealt onto; 0 (default) = one per slot.  With fewer streams than slots, slot i
                             enqueues on the stream of slot i % streams: several pairs QUEUED per stream.  The chip runs four hardware
                             queues well and no more, so a throughput host uses streams = 4 and slots = 8: a
                             stream's next pair is already enqueued when the one before it ends.  ugsm_wait(slot) still waits for
                             that slot's pair only. */
    int batch;            /* pairs per ugsm_submit_*_batch call the context expects (1 .. UGSM_MAX_BATCH; 0 = 1), and the size of the calls the
                             queue forms (ugsm_enqueue_*).  A slot's buffers are sized for it on first use (slots x batch x 1.35 GB at 16 MP,
                             ugsm_context_device_bytes) so that no reallocation lands between calls of different sizes; if that much memory
                             cannot be had the slot is sized for the call at hand instead, and a call that fits by itself still runs
                             (UGSM_ERR_NOMEM only if even that fails; a refused call leaves no buffer behind).  ugsm_plan_level reports the
                             kernels of a call of this many pairs. */
    int stream_priority;  /* HIP priority of the slots' streams.  0 (default): a pool of their own -- slots 0-3 at the GREATEST priority,
                             4-7 at the least, the rest at the process default: HIP deals streams onto 4 hardware queues PER PRIORITY
                             LEVEL, and two streams on one queue run strictly one after the other, so slots that share the default
                             pool with the host application's streams (the null stream any hipMemcpy uses, for a start) end up three
                             to a queue: 129 instead of 165 pairs/s at 16 MP.  The price: the library's kernels
                             are scheduled ahead of the host application's other GPU work, and a second context in the process (or
                             another process on the card) that does the same shares those four queues.  1: every slot at the
                             process default -- opt out, for a host whose own GPU work must not be outranked, or that runs several
                             contexts; 2: every slot at the greatest priority; 3: every slot at the least. */
} ugsm_config;

void ugsm_default_config(ugsm_config *cfg);
int ugsm_abi_version(void);
/* 0 in libugsm.so; 1 in libugsm_dev.so, the same sources built with the development kernels (include/ugsm_dev.h) */
int ugsm_is_dev_library(void);
const char *ugsm_status_string(int status);

/* MatchGPULib::MatchGPULib(argc, argv), MatchGPULib.cpp:251-265.  Owns all device
 * memory; reused across calls (the reference allocates/frees per level and resets
 * the device per call, :400).  Buffers grow on demand to the largest size seen. */
int ugsm_create(const ugsm_config *cfg, ugsm_ctx **out);
void ugsm_destroy(ugsm_ctx *ctx);
const char *ugsm_last_error(const ugsm_ctx *ctx);

/* ---- geometry / schedule (pure host; usable without a GPU) ---------------------- */

/* matching(): w[i+1] = (int)(w[i]/1.41421356), MatchGPULib.cpp:1224-1228 */
int ugsm_level_dims(int W, int H, int levels, int *w, int *h);
/* matchlevel(): mi = i>5 ? 22 : 2(i+1), MatchGPULib.cpp:1741 */
int ugsm_level_iterations(int level);
/* matchlevel(): realSmoothtime 10 for the two finest levels else 5, :2257-2261 */
int ugsm_level_smooth_passes(int level);
/* matchlevel(): clamp annealing, :1673 + :2299-2306; out[mi] */
int ugsm_threshold_schedule(int mi, float *out);
/* initStack()/getFoveaWidth()/getFoveaHeight(), MatchGPULib.cpp:406-426,268-274 */
int ugsm_fovea_dims(int W, int H, int levels, int fovea_levels, int *fovW, int *fovH);
/* Sum over levels of iterations x pixels; fovea_levels==0 => full-resolution mode */
long long ugsm_pixel_iterations(int W, int H, int levels, int fovea_levels);
/* The same for a seeded full-mode call (ugsm_submit_full_seeded): the levels start_level .. 0 only.  -1 for a size or a level that does not exist. */
long long ugsm_seeded_pixel_iterations(int W, int H, int levels, int start_level);
/* The same for the coarse half of a full-mode call (ugsm_submit_full_coarse): the levels stop_level .. levels - 1 only.  -1 for a size or a level
 * that does not exist.  For every e >= 1: ugsm_coarse_pixel_iterations(.., e) + ugsm_seeded_pixel_iterations(.., e - 1) is the whole call's. */
long long ugsm_coarse_pixel_iterations(int W, int H, int levels, int stop_level);
/* ... and for a warm foveated call (ugsm_submit_foveated_warm): fovW x fovH x the iterations of the levels start_level .. 0.  -1 likewise. */
long long ugsm_fovea_warm_pixel_iterations(int W, int H, int levels, int fovea_levels, int start_level);

/* Which kernels a W x H level runs under `cfg` (NULL = defaults), for maintainers and the host tests; results never depend on it.
 * ONE thing besides the level's size decides: whether the call has the chip to itself (`alone` != 0) or shares it with other calls.
 * The library answers that per call from what is in flight when the call is submitted -- nothing unfinished on any other slot and no
 * pairs waiting behind it in the queue -- so the blocking entry points (ugsm_match_*: the node's service call and its one-at-a-time
 * topic path) are alone whatever cfg->slots says, and the calls of a burst are not.  A call alone gets every launch as SHORT as possible
 * (nothing else fills the CUs a launch leaves idle: the coarse-level latency kernels up to 0.15 Mpx on their smallest tiles, K-smooth tile
 * heights that fill whole rounds of workgroups, the right pyramid and the A planes on a side stream -- an idle neighbour slot's stream,
 * borrowed for the call; a one-stream context has one stream more for it); a call that shares the
 * chip gets every launch doing little redundant work (latency kernels up to 50 k pixels only, on 18 x 18 tiles; one stream).
 * cost_kernel / smooth_kernel: 0 = LDS-tiled (k_smooth_fused; as a cost kernel: k_cost_split, libugsm_dev.so with march_min_pixels < 0 only), 1 = marching
 * (k_cost_march), 2 = coarse-level latency form (k_cost_small / k_smooth_small), 3 = one kernel per reference stage (kernel_path 1),
 * 4 (cost_kernel only) = channel-parallel marching form (k_cost_march4);
 * smooth_rh: region height of k_smooth_small (18, 24 or 32; else 0); strip_rows: rows per strip of the marching K-cost (else 0);
 * seed_fused: 1 if the level's seeding rides on its first K-cost launch; smooth_tile_rows: height of k_smooth_fused's 112-column
 * tile where that tile is used (else 0).  With cfg->batch > 1 the plan is that of a call of cfg->batch pairs (ugsm_submit_*_batch): every
 * threshold is compared with what the LAUNCH holds, pairs_per_launch x the level.  A configuration that ugsm_create would refuse (after the
 * same development overrides) has no plan: UGSM_ERR_BAD_ARG. */
typedef struct ugsm_level_plan {
    int cost_kernel, smooth_kernel, smooth_rh, strip_rows, seed_fused, smooth_tile_rows, alone;
    int pairs_per_launch;  /* ABI 4: cfg->batch where a call of that many pairs runs this level as one launch for all of them, else 1 */
} ugsm_level_plan;
int ugsm_plan_level(const ugsm_config *cfg, int alone, int W, int H, ugsm_level_plan *out);

/* ---- input formats: the byte layout of the images every entry point below reads ------------------------------------------------
 *
 * The node's image topics carry any encoding cv_bridge converts to rgb8 (UG_GPU_matcher.cpp:143-144,513-514); the library reads five of
 * them as they are.  A call on an image in format F gives, byte for byte, the result of the rgb8 call on that image converted the way
 * cv_bridge converts it to rgb8 -- disparities, confidence, fovea stacks, the L / R pyramid stacks, triangulated planes and the cloud's
 * colour word alike:
 *   UGSM_INPUT_RGB8   3 bytes per pixel, (b0, b1, b2) -- the default; every call made without ugsm_set_input_format reads this
 *   UGSM_INPUT_BGR8   3 bytes, R, G, B = (b2, b1, b0)
 *   UGSM_INPUT_RGBA8  4 bytes, (b0, b1, b2), alpha ignored
 *   UGSM_INPUT_BGRA8  4 bytes, (b2, b1, b0), alpha ignored
 *   UGSM_INPUT_MONO8  1 byte, (v, v, v)
 * `stride` stays bytes per row and must be at least ugsm_input_bytes_per_pixel(F) * W (UGSM_ERR_SIZE_MISMATCH otherwise; the cloud
 * calls answer UGSM_ERR_BAD_ARG, as for rgb8).  Device pointers of 8-bit images need no alignment (float images: below; the float buffers:
 * the last paragraph).
 * The format is a setting of the context that any call may change, and it is CAPTURED WHEN AN IMAGE IS HANDED OVER: by ugsm_match_*,
 * ugsm_submit_* (the pyramids, the shard), ugsm_stage_pyramid and the cloud calls when they are made, and by ugsm_enqueue_* for the pair
 * it enqueues -- the library forms the queue's calls later, each with the format its pairs were enqueued in (pairs of different formats
 * never share a call).
 *
 * FLOAT IMAGES.  The matcher's arithmetic is binary32 from its first line (the reference turns every 8-bit sample into a float,
 * MatchGPULib.cpp:332-338, and never reads a byte again), so an image that is float already -- a 12/16-bit camera scaled by its host
 * (mono16: v / 256, an exact power-of-two scale that keeps every bit), a pair rectified or normalised on the GPU, a 32FC1 / 32FC3 message --
 * is read as it stands:
 *   UGSM_INPUT_RGB32F   12 bytes per pixel: three binary32, (R, G, B)
 *   UGSM_INPUT_MONO32F   4 bytes per pixel: one binary32 v, read as (v, v, v)
 * The contract is the algorithm's: level 0 of the pyramid IS the given floats -- the conversion (float)byte is left out, nothing else
 * changes.  For images whose samples are finite and >= 0 every call that takes an image gives, bit for bit, what it gives on an 8-bit image
 * with level 0 equal to these floats: a float image whose samples are the integers 0 .. 255 gives the rgb8 (mono8) call's bytes on those
 * integers.  MONO32F is bit for bit RGB32F of (v, v, v), computed as one channel's passes.  The cloud calls' colour word takes each
 * channel as: NaN or v <= 0 -> 0, v >= 255 -> 255, else (uint8_t)(v + 0.5f).  Samples that are negative (-0.0 included), NaN or infinite:
 * every output is written, nothing is read or written out of bounds (a sample never indexes memory), and the values are UNSPECIFIED.
 * Image pointers stay `const uint8_t *` and `stride` bytes per row.  Beyond the refusals above, a float image whose pointer (device or
 * host) is not 4-byte aligned, or whose stride is no multiple of 4, is UGSM_ERR_BAD_ARG before anything is enqueued.  A float image is
 * four times the 8-bit one's bytes in the slots' image buffers and in the staging (16 MP rgb32f: 193 MB an image).
 * Not built: a planar (CHW) float layout; binary16 or 16-bit integer layouts; K-cost reading level 0 from a float image (a float call
 * materialises level 0, as bgr8 does); a defined result for negative or non-finite samples.
 *
 * ALIGNMENT OF FLOAT BUFFERS.  Every `float *` device buffer of this header, read or written -- d_out, d_stack, d_pyrL / d_pyrR, d_back,
 * d_prior, d_state, d_full, d_out3, d_xyz, the disparity, confidence and warp planes, the fields of the ugsm_stage_* entry points -- needs
 * 4-byte alignment and nothing more: a buffer at base + 4, + 8 or + 12 bytes of an allocation gives the same results bit for bit, and no
 * call writes outside the floats it is given (tests/test_gpu_caller_buffers.py).  The buffers that need more keep their refusals
 * (UGSM_ERR_BAD_ARG): d_points 16 bytes, the count words (d_count, d_level_counts, d_entry_counts) and the residual's sums 8 bytes. */
#define UGSM_INPUT_RGB8  0
#define UGSM_INPUT_BGR8  1
#define UGSM_INPUT_RGBA8 2
#define UGSM_INPUT_BGRA8 3
#define UGSM_INPUT_MONO8 4
#define UGSM_INPUT_RGB32F  8   /* 12 bytes per pixel: three binary32, (R, G, B) */
#define UGSM_INPUT_MONO32F 9   /*  4 bytes per pixel: one binary32 v, read as (v, v, v) */
/* 3, 3, 4, 4, 1 for the 8-bit formats, 12 and 4 for the float ones; -1 for an unknown format (5, 6, 7 and 10 among them).  Host only. */
int ugsm_input_bytes_per_pixel(int format);
/* The sensor_msgs encoding names "rgb8", "bgr8", "rgba8", "bgra8", "mono8", "32FC3" (RGB32F), "32FC1" (MONO32F) -> the format; -1 for any
 * other string and for NULL. */
int ugsm_input_format_from_encoding(const char *encoding);
/* UGSM_ERR_BAD_ARG for an unknown format (the format is left as it was).  Takes effect for the images handed over afterwards. */
int ugsm_set_input_format(ugsm_ctx *ctx, int format);
int ugsm_get_input_format(const ugsm_ctx *ctx, int *format);

/* ---- the LR check: which calls apply it ------------------------------------------------------------------------------------------
 *
 * The check is a setting of the context: a threshold tau and the set of calls that apply it.  ugsm_create leaves a context at
 * (ugsm_config.lr_check_threshold, UGSM_LR_FULL): the full-mode calls check, the foveated calls do not, as in every earlier ABI.
 *   UGSM_LR_FULL      ugsm_match_full, ugsm_submit_full[_host|_batch|_batch_host] and the full-mode queue: the pair is matched a second time
 *                     with the images exchanged (ugsm_config.lr_check_threshold above); batches run pair by pair.  (Both directions of a
 *                     full-mode batch in one lockstep call, the right camera's field returned too, tau per call and not from this
 *                     setting: ugsm_submit_full_checked.)
 *   UGSM_LR_FOVEATED  ugsm_match_foveated, ugsm_match_foveated_full, ugsm_submit_foveated[_host], ugsm_submit_foveated_batch[_host] and,
 *                     through those, ugsm_enqueue_foveated[_host|_managed].  (The multi-window call takes its check per call, not from
 *                     this setting: ugsm_submit_foveated_multi_checked.)
 * THE FOVEATED CHECK.  Let S be the stack of the call and B the stack of the same call with the two images exchanged -- the same offsets,
 * the same context: bit for bit what ugsm_submit_foveated(R, L, ..) returns.  The windows of L and R sit at the same coordinates, so level
 * k of S and level k of B live on one fovW x fovH grid, and each level k = 0 .. F-1 by itself is checked as ugsm_stage_lr_check checks a
 * fovW x fovH field: with sx = tex_index((ix + 0.5f) + dx, fovW) and sy likewise, both clamped to the window, the confidence of pixel
 * (ix, iy) becomes 0 where !(|dx + B.dx[sy][sx]| <= tau) or the same fails in y.  stackH, stackV and the pyramid stacks are untouched; B never
 * leaves the library; the check runs after the last level and never feeds back into the matching.  tau is in pixels OF THE LEVEL it is applied
 * to (a pixel of level k spans 1.41^k pixels of the image); a threshold per level is not offered.  ugsm_match_foveated_full reconstructs
 * from the checked stack: the zeros travel through the levels like any confidence.  A compact cloud (ugsm_point_cloud_fovea[_all],
 * min_conf > 0) of a checked stack leaves the marked pixels out.
 * What it costs: the right-to-left match is one more pair of the same call -- the same two pyramids, built once, with the L and R views
 * exchanged -- so a checked call of n pairs runs 2 n pairs through the levels in lockstep (as ugsm_submit_foveated_batch does, in launches of
 * at most UGSM_MAX_BATCH; the cost kernel alone takes one launch per direction), one launch checks the whole stack, and B lives in
 * 3 (F + 1) fovW fovH floats per pair of the slot (24 MB at 16 MP, counted by ugsm_context_device_bytes).  Measured on one MI355X: a
 * checked blocking call takes 1.73 x the plain one at 16 MP and 1.55 x at 1080p, where a second match would make it 2 x.
 * NOT checked, whatever the setting: ugsm_submit_fovea_coarse / _fine, ugsm_submit_fovea_shard and the ugsm_stage_* entry points.
 *
 * ugsm_set_lr_check: UGSM_ERR_BAD_ARG for !(tau >= 0) (the rule of ugsm_create) and for modes outside 0 .. 3; tau == 0 or modes == 0 switch
 * the check off, modes without UGSM_LR_FULL switch the full-mode check off (ugsm_last_lr_marked is then -1 after a full-mode call).
 * UGSM_LR_FOVEATED on a context with early_exit_threshold > 0 or kernel_path 1: UGSM_ERR_BAD_ARG -- those contexts run every level pair by
 * pair and have no batch dimension to carry the second direction in.  The setting is CAPTURED WHEN A SLOT-LEVEL CALL IS MADE; while pairs
 * enqueued with ugsm_enqueue_* are outstanding it cannot change (UGSM_ERR_STATE): set it before the first enqueue. */
#define UGSM_LR_FULL     1
#define UGSM_LR_FOVEATED 2
int ugsm_set_lr_check(ugsm_ctx *ctx, float tau, int modes);
int ugsm_get_lr_check(const ugsm_ctx *ctx, float *tau, int *modes);

/* ---- the service path: host buffers in, host buffers out ------------------------ */

/* MatchGPULib::match(L, R, 0), MatchGPULib.cpp:303-403, as used by
 * GPU_matcher::disparitySrv (UG_GPU_matcher.cpp:645-658) and mainRoutine (:423-442).
 * rgbL/rgbR: rgb8 rows of `stride` bytes (cv::Mat::step, :318), or the context's input format (ugsm_set_input_format).  dispH/dispV/dispC:
 * caller-allocated H*W float32 planes (the 32FC1 payloads of dispH/dispV/dispC). */
int ugsm_match_full(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H,
                    int stride, float *dispH, float *dispV, float *dispC);

/* MatchGPULib::matchStack / matchStackPyramid, MatchGPULib.cpp:429-700, plus the
 * node's stack packing (UG_GPU_matcher.cpp:293-320 disparity stacks, :203-226
 * pyramid stacks).  stackH/V/C: (fovea_levels*fovH) x fovW float32, level 0 (finest)
 * first.  pyrL/pyrR (may be NULL): (fovea_levels*3*fovH) x fovW, rows ordered
 * [level][channel][row].  off_x/off_y: fovea-centre offset from the image centre in
 * level-0 pixels; (0,0) is the reference's centred fovea (:1173-1176). */
int ugsm_match_foveated(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H,
                        int stride, int off_x, int off_y, float *stackH, float *stackV,
                        float *stackC, float *pyrL, float *pyrR);

/* MatchGPULib::match(L, R, fov == 1) (MatchGPULib.cpp:354-360): foveated matching followed by
 * hierarchicalDisparity (:2589-2701) -- one full-resolution (dx, dy, conf) field whose centre window comes from
 * the fine fovea levels and whose periphery from the coarser ones.  Host buffers as ugsm_match_full.
 * The reference node never takes this path (UG_GPU_matcher.cpp:421-423,644-645); SURVEY 8f row f-3. */
int ugsm_match_foveated_full(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H,
                             int stride, int off_x, int off_y, float *outH, float *outV, float *outC);

/* ---- throughput path: device buffers, asynchronous, one slot = one stream ------- */

/* Same computation as ugsm_match_full on device-resident inputs/outputs.
 * d_out: 3 contiguous H*W planes (dx, dy, conf).  Returns after enqueueing. */
int ugsm_submit_full(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR,
                     int W, int H, int stride, float *d_out);
/* Same as ugsm_match_foveated on device buffers; d_stack: 3 x (F*fovH) x fovW. */
int ugsm_submit_foveated(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR,
                         int W, int H, int stride, int off_x, int off_y, float *d_stack,
                         float *d_pyrL, float *d_pyrR);
/* ugsm_match_full without the wait, on any slot: for a host that keeps several pairs in flight from PAGE-LOCKED memory (SURVEY 8d:
 * "end-to-end from pinned host memory").  Every buffer -- both images and the three result planes -- must be page-locked
 * (ugsm_host_alloc, hipHostMalloc or hipHostRegister), else UGSM_ERR_BAD_ARG; the uploads, the match and the three downloads are
 * enqueued on the slot's stream and the call returns; ugsm_wait(slot) before the planes are read or the slot is used again. */
int ugsm_submit_full_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H,
                          int stride, float *dispH, float *dispV, float *dispC);
/* The same for ugsm_match_foveated (pyrL / pyrR may be NULL; page-locked if given). */
int ugsm_submit_foveated_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H,
                              int stride, int off_x, int off_y, float *stackH, float *stackV,
                              float *stackC, float *pyrL, float *pyrR);
/* B pairs per call (round 4) -- BASELINE configs[4] is "a batch of 8 x 16 MP foveated pairs"; the reference's loop is 176 strictly
 * sequential iterations per pair (MatchGPULib.cpp:1741-1743), and on every level of 615 x 407 pixels and below each of them is a launch
 * that lasts as long as ONE tile's or strip's chain whatever the rest of the chip could do.  The n pairs of a batch (1 <= n <=
 * UGSM_MAX_BATCH, all W x H) march through the levels in lockstep on the slot's stream: every level of at most 9 Mpx is ONE launch
 * for all of them (a pair index in every kernel's grid), larger levels fill the chip pair by pair and are launched so.  Same
 * arithmetic, same results bit for bit as n single calls.  d_rgbL / d_rgbR / d_out (d_stack, d_pyrL, d_pyrR): HOST arrays of n
 * DEVICE pointers, buffers laid out as for ugsm_submit_full / ugsm_submit_foveated; off_x / off_y: n window offsets (NULL = centred);
 * d_pyrL / d_pyrR may be NULL.  The slot holds the whole batch: ugsm_wait(slot) waits for all n pairs.  Contexts with
 * early_exit_threshold or lr_check_threshold set (and kernel_path 1) run the pairs one after the other. */
int ugsm_submit_full_batch(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                           int W, int H, int stride, float *const *d_out);
int ugsm_submit_foveated_batch(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                               int W, int H, int stride, const int *off_x, const int *off_y, float *const *d_stack,
                               float *const *d_pyrL, float *const *d_pyrR);
/* The same from PAGE-LOCKED host memory (as ugsm_submit_full_host / ugsm_submit_foveated_host): the uploads of all n pairs, one batched
 * match and the downloads of all results are enqueued on the slot's stream and the call returns; ugsm_wait(slot) before the results are read
 * or the slot is used again.  Every buffer page-locked, else UGSM_ERR_BAD_ARG.  (No pyramid stacks in the foveated form.) */
int ugsm_submit_full_batch_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR,
                                int W, int H, int stride, float *const *dispH, float *const *dispV, float *const *dispC);
int ugsm_submit_foveated_batch_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR,
                                    int W, int H, int stride, const int *off_x, const int *off_y, float *const *stackH,
                                    float *const *stackV, float *const *stackC);
/* The CHECKED full-mode call: both directions of n pairs (1 <= n <= UGSM_MAX_BATCH, all W x H) in one lockstep call, each pair's two fields
 * checked against each other.  tau (> 0, in pixels) is an argument of the call: the call neither reads nor changes what ugsm_set_lr_check holds.
 *   d_rgbL, d_rgbR, d_out  HOST arrays of n DEVICE pointers, buffers laid out as for ugsm_submit_full_batch.
 *   d_back                 the same for the right camera's checked field; may be NULL, and so may any of its entries: that pair's
 *                          right-to-left field then stays in the slot's LR buffer, as the context's own check keeps it.
 * The contract, bit for bit: d_out[k] is what ugsm_submit_full(L_k, R_k) writes on a context with ugsm_set_lr_check(ctx, tau, UGSM_LR_FULL),
 * d_back[k] what that same call writes for (R_k, L_k) -- dx and dy those of the unchecked matches, the confidence zeroed where the rule of
 * ugsm_stage_lr_check fails against the other direction's UNCHECKED dx and dy (neither check reads a confidence, so the two checks of a
 * pair do not depend on each other) -- in any input format, captured at the call.
 * How it runs: the pyramids of the n pairs are built once; the right-to-left match of pair k is one more entry of the same call that reads
 * pair k's pyramids with the L and R views exchanged, so 2 n full-frame fields run through the levels in lockstep -- every kernel of a level
 * of at most 9 Mpx one launch for all of them (launches of at most UGSM_MAX_BATCH entries; the cost kernel one launch per direction), larger
 * levels entry by entry -- level 0's last launch writes straight into d_out[k] and d_back[k], and ONE launch checks both directions of up
 * to eight pairs (nine to sixteen: two launches).  Cost against the context's own check, which matches the second direction after the first and single pairs only: DESIGN.md section 8.
 * Counts: ugsm_last_lr_marked_pair(ctx, slot, k, &fwd, &back) answers for pair k; ugsm_last_lr_marked the forward count of pair n-1;
 * ugsm_last_lr_marked_levels UGSM_ERR_STATE, as after any full-mode call.
 * Memory: the level buffers hold 2 n full fields -- 3 x 3 W H floats per pair more than the slot of an unchecked batch of n -- and the LR
 * buffer one field per pair whose d_back entry is NULL; both grow on demand, counted by ugsm_context_device_bytes.
 * Status, all before anything is enqueued: !(tau > 0), NaN included, null arrays, null entries of d_rgbL / d_rgbR / d_out, n outside
 * 1 .. UGSM_MAX_BATCH: UGSM_ERR_BAD_ARG; contexts with early_exit_threshold > 0 or kernel_path 1: UGSM_ERR_BAD_ARG (ugsm_set_lr_check's rule for
 * the lockstep check: they have no batch dimension); the size errors of ugsm_submit_full as there; pairs outstanding in the queue:
 * UGSM_ERR_STATE; a buffer that cannot grow: UGSM_ERR_NOMEM, the context usable afterwards.
 * The queue form: ugsm_enqueue_full_checked[_managed | _cloud | _cloud_managed], below ("checked pairs through the queue"); from page-locked
 * memory: ugsm_submit_full_checked_host.
 * NOT built: a seeded or coarse / fine checked call; of the queue form, the page-locked _host kind (device and managed pairs only).
 * Asynchronous on `slot`. */
int ugsm_submit_full_checked(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                             int W, int H, int stride, float *const *d_out, float *const *d_back, float tau);
/* The same call from page-locked host memory, in and out, as ugsm_submit_full_batch_host: the images of the n pairs go up, both directions run
 * in lockstep, the checked forward planes come down into dispH / dispV / dispC [k], and the right camera's checked planes into backH / backV /
 * backC [k] for the pairs that ask for them -- the three arrays NULL (no pair asks), or all three given with, per pair, all three entries set
 * or all three NULL; anything else is UGSM_ERR_BAD_ARG.  Every buffer page-locked, else UGSM_ERR_BAD_ARG.  The planes are the fields of
 * ugsm_submit_full_checked, bit for bit; its refusals, counts and memory, plus one device field per pair (two for a pair that takes its back
 * planes) of result staging in the slot.  Asynchronous on `slot`: every buffer stays valid and untouched until ugsm_wait(ctx, slot). */
int ugsm_submit_full_checked_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR,
                                  int W, int H, int stride, float *const *dispH, float *const *dispV, float *const *dispC,
                                  float *const *backH, float *const *backV, float *const *backC, float tau);
/* Blocking, one pair, any host memory in and out, as ugsm_match_full.  backH / backV / backC (the right camera's checked planes): all three
 * or none (NULL); anything else is UGSM_ERR_BAD_ARG. */
int ugsm_match_full_checked(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                            float *dispH, float *dispV, float *dispC, float *backH, float *backV, float *backC, float tau);
/* The SEEDED full-mode call: n pairs (1 <= n <= UGSM_MAX_BATCH, all W x H) matched from level start_level downwards, each from a prior field of
 * its own instead of from the zero seed at the top level -- for a host that matched the previous frame and so holds a field better than
 * anything the coarse levels can produce (a tracker, a video pipeline).  The reference has nothing like it: the build's own definition, as the
 * LR check is.
 *   d_rgbL, d_rgbR, d_out  HOST arrays of n DEVICE pointers, buffers laid out as for ugsm_submit_full_batch.
 *   d_prior                the same for the priors: full-resolution fields (3 planes of W x H: dx, dy, conf), e.g. an earlier call's d_out.
 *   start_level            0 .. levels - 1: the first level that is matched.
 * The contract, bit for bit: d_out[k] is the field reached by restricting d_prior[k] to level start_level, running matchlevel on the levels
 * start_level .. 0 with the usual iteration and smoothing counts and subsampleDisp between them, and never taking the top level's
 * first-iteration exception: level start_level's first iteration blends the confidence like any other, because a prior has one.
 * The restriction (ugsm_stage_restrict runs it alone) reads the prior at the sites the image pyramid samples level s's pixels from.  With
 * k = s / 2: for an even s column x reads column ((x + 1) << k) - 1 -- k steps of the pyramid's sf = 2.0f sampling tex_index((c + .5f) * 2) --;
 * for an odd s first c1 = ((x + 1) << k) - 1, a level-1 column, then tex_index((c1 + 0.5f) * (float)1.41421356, W), the pyramid's
 * level-0 -> level-1 sampling; rows likewise.  dx and dy of an odd level become q = (float)((double)v / 1.41421356), the partner of
 * subsampleDisp's SCALE * v, then q * 2^-k in binary32; of an even level v * 2^-k; the confidence is copied; s = 0 is a copy.
 * What runs: the pyramid kernels build the levels 0 .. max(start_level, 2) only; one restriction launch fills level start_level's fields where
 * the zero seed is otherwise set; the levels above run nothing; from level start_level downwards every launch is the full-mode call's -- the n
 * pairs in lockstep exactly as ugsm_submit_full_batch groups them, level 0 from the images where it does so.  Any input format, captured at
 * the call.  d_prior[k] == d_out[k] is allowed (the restriction reads before level 0 writes, on the same stream), and a prior that is the
 * d_out of the call enqueued just before on the same slot needs no wait in between.
 * NOT the cold call: a seeded call from the top level with a zero prior differs from ugsm_submit_full because of the blend.  A cold start from
 * level s is a context with levels = s + 1.
 * Status, all before anything is enqueued: null arrays or null entries, n outside 1 .. UGSM_MAX_BATCH, start_level outside 0 .. levels - 1,
 * contexts with early_exit_threshold > 0: UGSM_ERR_BAD_ARG; UGSM_LR_FULL in force (ugsm_set_lr_check) or pairs outstanding in the queue:
 * UGSM_ERR_STATE; the size errors of ugsm_submit_full as there.  kernel_path 1 (libugsm_dev.so) runs the pairs one after the other, as it does
 * for ugsm_submit_full_batch.  What it saves, measured: DESIGN.md section 8.
 * NOT built: a queue form (ugsm_enqueue_*); the page-locked _host kind; a seeded checked or foveated call of this kind (the foveated one is
 * a call of its own, from a prior STACK: ugsm_submit_foveated_warm, below).
 * Asynchronous on `slot`. */
int ugsm_submit_full_seeded(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                            int W, int H, int stride, const float *const *d_prior, int start_level, float *const *d_out);
/* Blocking, one pair on slot 0, any host memory in and out, as ugsm_match_full; the prior: three planes of W x H, not the result planes. */
int ugsm_match_full_seeded(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                           const float *priorH, const float *priorV, const float *priorC, int start_level,
                           float *dispH, float *dispV, float *dispC);
/* The seeded FOVEATED call -- "warm", against the cold call that starts from the zero seed at the top level: n pairs (1 <= n <= UGSM_MAX_BATCH,
 * all W x H) matched from FOVEA level start_level downwards, each from a prior fovea STACK of its own, whose window may lie elsewhere than the
 * new one -- for a tracker, which looks at one place frame after frame and holds the previous frame's stack for it.  Every matched level of a
 * stack is a fovW x fovH field, so a foveated call is launch-bound throughout and the coarse levels it leaves out are most of its launches.
 * The build's own definition, as ugsm_submit_full_seeded is.
 *   d_rgbL, d_rgbR, off_x, off_y, d_stack  as ugsm_submit_foveated_batch takes them (a NULL offset array: centred); no pyramid stacks.
 *   d_prior_stack              HOST array of n DEVICE pointers: stacks of the d_stack layout, e.g. an earlier call's d_stack.
 *   prior_off_x, prior_off_y   the offsets those stacks were matched at (NULL: centred).
 *   start_level                0 .. fovea_levels - 1: the first level that is matched.
 * The starting fields, from operations this header already defines (so every comparison is bit for bit): with P the full-resolution field
 * ugsm_reconstruct_full gives for the prior stack at the prior's offsets, and R_k what ugsm_stage_restrict gives for P at level k, the
 * starting field of level k (start_level <= k <= F-1) is the fovW x fovH crop of R_k at the NEW window's origin at level k (level F-1: the
 * whole level).  ONE launch computes them pointwise from the stack (ugsm_stage_warm_stack runs it alone): neither P -- twice 193 MB written at
 * 16 MP -- nor R_k is ever formed.  For a target pixel: its level-0 site (sx, sy) as in ugsm_submit_full_seeded's restriction; then V_0(sx, sy),
 * where V_{F-1}(x, y) is row block F-1 of the prior at (x, y) and, for l < F-1, V_l(x, y) is row block l at (x - ox_l, y - oy_l) where that
 * lies inside the prior's window of level l, else (float)1.41421356 * V_{l+1}(tex((x + .5f) / (float)1.41421356), tex((y + .5f) / ...)) --
 * ugsm_reconstruct_full's step, all three channels scaled, every multiplication rounded on its own --; then the restriction's value transform.
 * The contract, bit for bit: row blocks start_level + 1 .. F-1 of d_stack[k] receive their starting fields -- the prior carried over to the new
 * window by ONE rule (no copy-if-the-window-did-not-move branch: inside a finer window of the prior the finer level's value is the better one),
 * so the result is itself a valid prior and a valid input to ugsm_reconstruct_full and the cloud calls.  Level start_level is matched from its
 * starting field with its usual iteration and smoothing counts and never takes the top level's first-iteration exception; the levels below
 * follow exactly as the fine phase of ugsm_submit_foveated runs them (foveatedsubsampleDisp between them, the window views of the new
 * offsets); start_level = F-1 matches the whole-frame level F-1 first.  Row blocks 0 .. start_level receive the matched fields.  Nothing else
 * is written.
 * What runs: the pyramid kernels build the levels 0 .. max(start_level, 2) only, level 0 inside the windows; one starting-field launch per
 * call (k_restrict_stack in the kernel statistics, at level start_level, n (F - start_level) fovW fovH pixel-launches); no launch at any level
 * above start_level; from there down every launch is the one ugsm_submit_foveated_batch makes for these n pairs, lockstep grouping included.
 * Any input format, captured at the call.  A call whose prior is the d_stack of the call enqueued just before on the same slot needs no wait
 * in between.
 * WARNING: a chain of warm calls never refreshes the levels above start_level -- they are carried over, resampled, frame after frame.  The host
 * decides when to run a cold call (ugsm_submit_foveated) again.
 * Status, all before anything is enqueued: null arrays or null entries, n outside 1 .. UGSM_MAX_BATCH, start_level outside 0 .. F-1,
 * fovea_levels < 2, contexts with early_exit_threshold > 0, and a prior that overlaps one of the call's d_stack buffers (the call is NOT in
 * place: the launch that reads the priors writes the stacks; a tracker alternates two stacks, 21 MB each at 16 MP): UGSM_ERR_BAD_ARG;
 * UGSM_LR_FOVEATED in force (ugsm_set_lr_check) or pairs outstanding in the queue: UGSM_ERR_STATE; the size errors of ugsm_submit_foveated as
 * there.  kernel_path 1 (libugsm_dev.so) runs the pairs one after the other.  What it saves, measured: DESIGN.md section 8.
 * NOT built: pyramid stacks from this call (the levels above max(start_level, 2) are not built); a queue or managed form; the page-locked
 * _host kind; a checked call; a multi-window call; start levels above F-1.
 * Asynchronous on `slot`. */
int ugsm_submit_foveated_warm(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                              const int *off_x, const int *off_y, const float *const *d_prior_stack, const int *prior_off_x, const int *prior_off_y,
                              int start_level, float *const *d_stack);
/* The same from full-resolution FIELDS (3 planes of W x H each, e.g. a full-mode d_out) -- for the host that matches the whole frame once
 * and follows windows afterwards: P is the field itself and the descent above has depth zero. */
int ugsm_submit_foveated_warm_field(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                                    const int *off_x, const int *off_y, const float *const *d_prior_field, int start_level, float *const *d_stack);
/* Blocking, one pair on slot 0, any host memory in and out, as ugsm_match_foveated; the prior: the three planes of a stack, not the result planes. */
int ugsm_match_foveated_warm(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                             const float *priorH, const float *priorV, const float *priorC, int prior_off_x, int prior_off_y, int start_level,
                             float *stackH, float *stackV, float *stackC);
/* The full-mode call in TWO HALVES: stop at level e, resume from its field -- for a host that wants a field at reduced resolution from
 * full-resolution images (a preview, an obstacle map, a fovea controller that decides where to look) and, perhaps later, the full one without
 * starting again at the top level.  The levels 6 .. 13 hold 8 % of a call's pixel-iterations and most of its launches, the levels 0 and 1
 * about half of its work.  Below: w[], h[] by ugsm_level_dims, top = levels - 1.
 * The contract, bit for bit: coarse(e) followed by fine(e) is ugsm_submit_full.
 *
 * COARSE.  n pairs (1 <= n <= UGSM_MAX_BATCH, all W x H); d_rgbL, d_rgbR, d_state, d_full: HOST arrays of n DEVICE pointers.
 *   d_state[k]  receives three planes (dx, dy, conf) of w[e] x h[e], e = stop_level (0 .. top): the field of level e after matchlevel on the
 *               levels top .. e from the zero seed, subsampleDisp between them, the top level with its first-iteration exception -- what the
 *               cold call holds in its level buffer when level e has finished.  stop_level = 0 is ugsm_submit_full_batch.
 *   d_full      may be NULL, and so may any of its entries; where d_full[k] is given it receives three planes of W x H: the PROLONGATION of
 *               d_state[k], P_0 of
 *                   P_l[y][x] = (float)(1.41421356 * (double)P_l+1[tex(((float)y + 0.5f) * sf, h[l+1])][tex(((float)x + 0.5f) * sf, w[l+1])])
 *               for l = e-1 .. 0, with P_e the state, sf = (float)(1 / 1.41421356) and tex the matcher's texture index (floor; NaN or negative:
 *               0; clamped to n - 1) -- e steps of subsampleDisp without a crop (ugsm_stage_seed).  All three planes are scaled: the reference
 *               scales the confidence too.  e = 0 is a copy.  Every level's own size takes part: the clamp binds at some levels (for 333
 *               columns on the steps from the levels 0, 2, 3, 4, 7, 8, 10, 12) and there is no closed form.  A prolonged field is a W x H field
 *               like any other: for the clouds, the warp, the residual, and for ugsm_submit_full_seeded as a prior.
 * What runs: the pyramids as ugsm_submit_full_batch builds them; every launch of the levels top .. e is the one that call makes for these n
 * pairs, lockstep grouping and a lone pair's A planes from the side stream included; no K-cost, K-smooth, A or seed launch at any level below e;
 * ONE prolongation launch per call for all the pairs with a d_full entry (k_prolong in the kernel statistics, at level e, pairs x W x H
 * pixel-launches; ugsm_stage_prolong runs it alone), which computes P_0 pointwise -- P_1 .. P_e-1 are never formed.  Any input format, captured
 * at the call.  Nothing is written past the three planes of either output.
 *
 * FINE.  d_state[k]: a field of level e = state_level (1 .. top), three planes of w[e] x h[e]; d_out[k] receives the field reached by
 * subsampleDisp of the state to level e - 1, then matchlevel on the levels e-1 .. 0 with their usual iteration and smoothing counts and
 * subsampleDisp between them; no level takes the top level's exception.  With the d_state of ugsm_submit_full_coarse(.., e, ..) for the same
 * pair on a context of the same `levels`, d_out[k] is bit for bit ugsm_submit_full's result -- for every e, however the n pairs are grouped,
 * in any input format.  A state from anywhere else (another frame's, another process's, one the host wrote) is allowed: the definition says
 * what comes out.
 * What runs: the pyramid kernels build the levels 0 .. max(e - 1, 2) only, as the seeded call's; one device-to-device copy per pair places the
 * state in the level buffer (at most 3 w[1] h[1] floats); the step to level e - 1 is the cold call's own -- fused into that level's first K-cost
 * launch where the call fuses it, k_seed otherwise --; from level e - 1 down every launch is the full-mode batch call's, level 0 from the images
 * where it reads them, its last smoothing launch writing d_out[k].  The state is read before anything of the call is written, on the slot's
 * stream: a state that is the d_state of a coarse call enqueued just before on the same slot needs no wait in between.
 *
 * Status, all before anything is enqueued (a refused call writes nothing): null arrays, null entries of d_rgbL / d_rgbR / d_state / d_out,
 * n outside 1 .. UGSM_MAX_BATCH, stop_level outside 0 .. top, state_level outside 1 .. top, contexts with early_exit_threshold > 0, a d_full[k]
 * that overlaps any of the call's states: UGSM_ERR_BAD_ARG; UGSM_LR_FULL in force (ugsm_set_lr_check) or pairs outstanding in the queue:
 * UGSM_ERR_STATE; the size errors of ugsm_submit_full as there.  kernel_path 1 (libugsm_dev.so) runs the pairs one after the other (and then
 * one prolongation per pair).  What the halves cost, measured: DESIGN.md section 8, "The call in two halves".
 * NOT built: a queue or managed form (ugsm_enqueue_*); the page-locked _host kind; a checked or seeded coarse call; the node's use of it;
 * clouds straight from a level-sized state (prolong it first).
 * Both asynchronous on `slot`. */
int ugsm_submit_full_coarse(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                            int W, int H, int stride, int stop_level, float *const *d_state, float *const *d_full);
int ugsm_submit_full_fine(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR,
                          int W, int H, int stride, const float *const *d_state, int state_level, float *const *d_out);
/* Blocking, one pair on slot 0, any host memory in and out, as ugsm_match_full.  state*: planes of w[e] x h[e]; fullH / fullV / fullC (planes
 * of W x H, the prolongation): all three or none (NULL), anything else is UGSM_ERR_BAD_ARG. */
int ugsm_match_full_coarse(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int stop_level,
                           float *stateH, float *stateV, float *stateC, float *fullH, float *fullV, float *fullC);
int ugsm_match_full_fine(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                         const float *stateH, const float *stateV, const float *stateC, int state_level,
                         float *dispH, float *dispV, float *dispC);
/* ---- several fovea windows on ONE pair ------------------------------------------------------------------------------------------------
 *
 * A host that looks at n places of one frame (1 <= n <= UGSM_MAX_BATCH) needs the pyramids and the coarse phase -- levels top .. F-1, which
 * do not depend on the window -- once, and the fine levels F-2 .. 0 of its n windows: those run in lockstep, as the pairs of
 * ugsm_submit_foveated_batch do, every kernel of a level one launch for all n windows.  Level 0 is stored inside the windows alone.
 *   off_x / off_y  n window offsets (NULL = all centred).  Offsets that clamp at the frame, duplicates and overlapping windows are allowed.
 *   d_stack        HOST array of n DEVICE stacks, each 3 x (F*fovH) x fovW as ugsm_submit_foveated writes it.
 * The matching contract: stack k is, bit for bit, what ugsm_submit_foveated(ctx, slot, d_rgbL, d_rgbR, .., off_x[k], off_y[k], d_stack[k],
 * NULL, NULL) writes -- for any n, in any input format (ugsm_set_input_format, captured at the call); row block F-1 of every stack is the same
 * whole-frame level.  With n == 1 the call IS ugsm_submit_foveated without pyramid stacks.
 * Status: null arrays or entries, n outside 1 .. UGSM_MAX_BATCH, fovea_levels < 2: UGSM_ERR_BAD_ARG; the size errors of ugsm_submit_foveated
 * as there; pairs outstanding in the queue: UGSM_ERR_STATE; UGSM_LR_FOVEATED set on the context: UGSM_ERR_STATE (the checked multi-window
 * call is an entry point of its own, ugsm_submit_foveated_multi_checked below).  All of these before anything is enqueued.
 * Memory: one pair's slot, plus level buffers that hold n fields of 3 fovW fovH floats -- more than a one-pair slot has once n > 2^(F-1); they
 * grow on demand (counted by ugsm_context_device_bytes), and a call whose buffers cannot grow answers UGSM_ERR_NOMEM.
 * After the call the slot holds no whole pyramids: ugsm_submit_fovea_fine on it answers UGSM_ERR_STATE, as after any one-shot foveated call.
 * Contexts with early_exit_threshold set, and kernel_path 1, still build the pyramids and run the coarse phase once; their n fine phases run
 * one after the other.  Same results.
 * NOT built: pyramid stacks from this call; a queue form (ugsm_enqueue_*); the page-locked _host kind.  The merged cloud of the n stacks is
 * ugsm_point_cloud_fovea_multi (below, with the other clouds).
 * Asynchronous on `slot`. */
int ugsm_submit_foveated_multi(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride,
                               int n, const int *off_x, const int *off_y, float *const *d_stack);
/* Blocking, any host memory in, host stacks out (HOST arrays of n pointers each), as ugsm_match_foveated; no pyramid stacks. */
int ugsm_match_foveated_multi(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                              int n, const int *off_x, const int *off_y, float *const *stackH, float *const *stackV,
                              float *const *stackC);
/* The CHECKED multi-window call: both directions of the n windows in one lockstep call, the n stacks checked against their right-to-left twins.
 * tau (> 0, in pixels of the level it is applied to) is an argument of the call: the call neither reads nor changes what ugsm_set_lr_check
 * holds, and runs the same with UGSM_LR_FOVEATED set or not.
 * The contract: stack k is, bit for bit, what ugsm_submit_foveated(ctx, slot, d_rgbL, d_rgbR, .., off_x[k], off_y[k], d_stack[k], NULL, NULL)
 * writes on a context with ugsm_set_lr_check(ctx, tau, UGSM_LR_FOVEATED) -- stackH and stackV those of the unchecked call, stackC of level j
 * zeroed where the rule of "THE FOVEATED CHECK" fails against the stack of the exchanged pair at the same offset; row block F-1 the same
 * checked whole-frame level in every stack -- for any n in 1 .. UGSM_MAX_BATCH, any input format captured at the call, and offsets that clamp,
 * repeat or overlap.  The pyramids are built once and the coarse phase runs once for the two directions; the right-to-left stacks never leave
 * the library (the slot's LR buffer, counted by ugsm_context_device_bytes; the level buffers hold 2 n fovea fields and grow on demand).
 * Counts: ugsm_last_lr_marked_levels(ctx, slot, k, per_level) answers for window k (pair >= n: UGSM_ERR_BAD_ARG); ugsm_last_lr_marked the
 * levels of window n-1.  After a plain ugsm_submit_foveated_multi on the slot both answer as after any unchecked call.
 * Status, all before anything is enqueued: !(tau > 0), NaN included: UGSM_ERR_BAD_ARG; contexts with early_exit_threshold > 0 or kernel_path 1:
 * UGSM_ERR_BAD_ARG (ugsm_set_lr_check's rule: they have no batch dimension); every refusal of ugsm_submit_foveated_multi as it stands there but
 * the one about UGSM_LR_FOVEATED; a buffer that cannot grow: UGSM_ERR_NOMEM, the context usable afterwards.
 * NOT built: a queue form; the page-locked _host kind; pyramid stacks. */
int ugsm_submit_foveated_multi_checked(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride,
                                       int n, const int *off_x, const int *off_y, float *const *d_stack, float tau);
/* Blocking, any host memory in, host stacks out, as ugsm_match_foveated_multi. */
int ugsm_match_foveated_multi_checked(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                                      int n, const int *off_x, const int *off_y, float *const *stackH, float *const *stackV,
                                      float *const *stackC, float tau);
int ugsm_wait(ugsm_ctx *ctx, int slot);
/* ugsm_wait on every slot, in order; every slot is waited for whatever the ones before it answered, the first failure is the one returned. */
int ugsm_wait_all(ugsm_ctx *ctx);
/* The HIP stream `slot` enqueues on (a hipStream_t, returned as a plain pointer): lets a host that owns other streams -- the
 * RCCL collective of the fovea shard -- order them after the slot's work ON THE DEVICE (record an event on this stream, make the
 * other stream wait for it) instead of blocking in ugsm_wait.  The stream stays owned by the context. */
int ugsm_slot_stream(ugsm_ctx *ctx, int slot, void **hip_stream);
/* Non-blocking ugsm_wait: UGSM_OK when everything enqueued on `slot` has finished (its launch statistics are harvested, as by
 * ugsm_wait), UGSM_PENDING while it has not. */
int ugsm_poll(ugsm_ctx *ctx, int slot);

/* ---- the queue: the library owns the slots (round 5) -------------------------------------------------------------------------------
 *
 * What a host needs for THROUGHPUT is not "a call of n pairs on slot s" but "here is another pair; tell me when it is done": which
 * pairs share a call, which slot takes it and when a slot is free again is the library's business.  (Rounds 3-4 kept that logic in the
 * benchmark harness -- bench.py's plan_calls / run / submit -- where no user of this header could reach it.)  The reference node's
 * topic path (UG_GPU_matcher.cpp:126-185,414-494: one blocking match() per synchronised image pair inside a single-threaded
 * ros::spin, :749-752) becomes enqueue-on-arrival + publish-on-completion with `frames_in_flight` pairs outstanding
 * (ros/UG_GPU_matcher_ugsm.cpp, ug_stereomatcher_amd/service.py); results are reported strictly in the order the pairs were enqueued.
 *
 * ugsm_enqueue_* appends one pair to the context's backlog and returns; it never waits for that pair.  Calls are formed from the
 * backlog by one rule ("batch what has piled up"):
 *   - a call goes out as soon as `target` pairs of one kind (mode, memory kind, W x H, stride) wait, where target = ugsm_config.batch,
 *     except for the first `slots` calls of a burst (after ugsm_create, and after every flush), which are staggered -- call c takes
 *     ceil(batch (c + 2) / (slots + 1)) pairs (4, 5, 7, 8 for batch 8 on four slots) so that the slots do not march through the pyramid
 *     levels in phase from a drained pipe ("The queue");
 *   - ugsm_flush, or a blocking ugsm_next_done, declares that nothing more is coming for now: whatever waits goes out in calls of at
 *     most `target` pairs as slots come free, without waiting for a call to fill.  A host that wants every frame started at once calls
 *     ugsm_flush after every ugsm_enqueue_*: calls then hold one pair while slots are free and grow by themselves under load;
 *   - a pair of another kind than the ones waiting sends those out first (a call holds pairs of one kind).
 * Slots are used in rotation; a free slot is preferred, else the call waits (inside ugsm_enqueue_*: back-pressure) for the slot that
 * holds the oldest call.  At most (slots + 1) x batch pairs are outstanding -- enqueued and not yet reported by ugsm_next_done -- at
 * any time: a host that recycles (slots + 1) x batch result buffers in enqueue order never overwrites a result it has not been told
 * about.  A host that lets completions pile up unfetched until that many are outstanding gets UGSM_ERR_STATE from ugsm_enqueue_*
 * (nothing is enqueued; fetch with ugsm_next_done and try again).
 * The library makes progress only inside its own entry points (no thread of its own): calls go out and completions are noticed during
 * ugsm_enqueue_*, ugsm_flush and ugsm_next_done.  While pairs are outstanding the slots belong to the queue: the slot-level entry points
 * (ugsm_submit_*, ugsm_match_*, ugsm_stage_*) answer UGSM_ERR_STATE until every pair has been reported.
 * Results are identical, bit for bit, to single calls of ugsm_submit_full / ugsm_submit_foveated on the same inputs, however the pairs
 * were grouped. */
typedef struct ugsm_completion {
    uint64_t tag;          /* the host's name for the pair (ugsm_enqueue_*) */
    int status;            /* UGSM_OK, or the status of the library call the pair went out in */
    int slot;              /* slot that ran it */
    int call_pairs;        /* pairs of that call ... */
    int reserved;
    long long call_index;  /* ... and its running number since ugsm_create */
    long long done_ns;     /* CLOCK_MONOTONIC, nanoseconds, when the library noticed the call complete */
    float *result[5];      /* ugsm_enqueue_*_managed only (else NULL): page-locked planes owned by the library, valid until the NEXT
                              ugsm_next_done on this context -- full mode: dispH, dispV, dispC (H x W each); foveated: stackH, stackV, stackC
                              ((F fovH) x fovW each), then the L and R pyramid stacks ((F 3 fovH) x fovW) if they were asked for */
} ugsm_completion;

/* Return value of every ugsm_enqueue_*: UGSM_OK = the pair is ACCEPTED -- it will be reported by ugsm_next_done exactly once, whatever
 * happens to the call it goes out in; anything else = the pair is REJECTED and nothing was enqueued (bad arguments, buffers that are not
 * page-locked, UGSM_ERR_STATE when (slots + 1) x batch pairs are outstanding, UGSM_ERR_NOMEM for the library's own bookkeeping or staging).
 * A library call that fails -- e.g. UGSM_ERR_NOMEM when the slot's buffers cannot be had -- is reported through ugsm_completion.status of
 * each of its pairs and nowhere else: the call an enqueue happens to send may hold OTHER pairs than the one just appended.  A failed call's
 * pairs are reported only after whatever the call did put on the slot's stream has drained, so a completion always means that the pair's
 * input and result buffers are no longer in use.
 * Device buffers (as ugsm_submit_full / ugsm_submit_foveated; d_pyrL / d_pyrR may be NULL).  Inputs and outputs must stay valid and
 * untouched until the pair's tag has been reported by ugsm_next_done. */
int ugsm_enqueue_full(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out, uint64_t tag);
int ugsm_enqueue_foveated(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int off_x, int off_y,
                          float *d_stack, float *d_pyrL, float *d_pyrR, uint64_t tag);
/* PAGE-LOCKED host buffers (as ugsm_submit_full_host / ugsm_submit_foveated_host; UGSM_ERR_BAD_ARG if any is not): uploads, match
 * and downloads are enqueued with the call the pair goes out in.  Same lifetime rule. */
int ugsm_enqueue_full_host(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH, float *dispV,
                           float *dispC, uint64_t tag);
int ugsm_enqueue_foveated_host(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                               float *stackH, float *stackV, float *stackC, float *pyrL, float *pyrR, uint64_t tag);
/* Any host memory in, library-owned results out: the images are copied into page-locked staging memory of the context BEFORE the call
 * returns (the caller's buffers -- a ROS message's payload -- may be freed at once), the results land in page-locked planes the library
 * lends to the host through ugsm_completion.result.  This is what the node's topic path uses: no page-locked memory to manage, no
 * result planes to allocate per frame (the reference mallocs and frees 193 MB per 16 MP frame, UG_GPU_matcher.cpp:414-418,487-489).
 * want_pyramids: also return the L / R fovea pyramid stacks (matchStackPyramid, MatchGPULib.cpp:534-700). */
int ugsm_enqueue_full_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, uint64_t tag);
int ugsm_enqueue_foveated_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                                  int want_pyramids, uint64_t tag);
/* "Nothing more is coming for now": every pair waiting at this moment goes out as slots allow, without waiting for its call to fill.
 * Never blocks: pairs no slot is free for stay queued and go out inside a later ugsm_enqueue_* / ugsm_next_done. */
int ugsm_flush(ugsm_ctx *ctx);
/* The oldest pair not yet reported.  UGSM_OK: *out filled (out->status tells how its call went).  block = 0: UGSM_PENDING if that pair
 * has not finished (or has not gone out yet), UGSM_EMPTY if there is none.  block != 0: implies ugsm_flush, waits for the pair;
 * UGSM_EMPTY only if nothing is outstanding. */
int ugsm_next_done(ugsm_ctx *ctx, ugsm_completion *out, int block);
/* Pairs waiting in the backlog, pairs in calls that are in flight (as far as the library has noticed), completions not yet fetched. */
int ugsm_queue_depth(ugsm_ctx *ctx, int *waiting, int *in_flight, int *unreported);
/* Host only: the calls the queue of a context created with `cfg` (NULL = defaults) forms from a burst of n_pairs pairs of one kind
 * enqueued back to back from idle and then flushed -- sizes[0 .. return value) (cap entries at most are written; the return value is
 * the number of calls, or -1 for bad arguments).  20 pairs, batch 8, four slots: 4, 5, 7, 4. */
int ugsm_queue_plan(const ugsm_config *cfg, int n_pairs, int *sizes, int cap);

/* Fovea sharding over several GPUs (north-star; no reference counterpart: the
 * reference has one centred fovea on one GPU).  coarse: pyramids + levels
 * top..F-1 on the full frame; d_state receives level F-1's (dx,dy,conf),
 * 3*fovH*fovW floats -- the 3 MB object broadcast over RCCL.  fine: levels
 * F-2..0 for the window at (off_x, off_y) from a (possibly received) d_state;
 * needs the pair's WHOLE pyramids in the slot, i.e. ugsm_submit_pyramids first (UGSM_ERR_STATE otherwise; a full-mode call leaves none
 * behind: it reads level 0 from the images themselves and may not store it).  The one-shot foveated
 * calls (ugsm_match_foveated, ugsm_submit_foveated[_batch|_host]) know their windows when they build the pyramids and store level 0
 * only inside them (CreateFoveatedPyramid crops after a full build, MatchGPULib.cpp:1128-1190; here 193 MB per 16 MP image are never
 * written), so their pyramids do NOT serve a later ugsm_submit_fovea_fine at another offset. */
int ugsm_submit_pyramids(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR,
                         int W, int H, int stride);
int ugsm_submit_fovea_coarse(ugsm_ctx *ctx, int slot, float *d_state);
int ugsm_submit_fovea_fine(ugsm_ctx *ctx, int slot, const float *d_state, int off_x, int off_y,
                           float *d_stack);

/* ---- the fovea shard with its exchange inside the library (round 5): RCCL on the slot's own stream ---------------------------------
 *
 * One process (or one context) per GPU; the contexts of a shard form ONE RCCL communicator.  ugsm_submit_fovea_shard enqueues, on the
 * slot's stream and nowhere else: the pair's pyramids; on rank `src_rank` the coarse full-frame levels top .. F-1
 * (ugsm_submit_fovea_coarse); ncclBroadcast of level F-1's (dx, dy, conf) -- 3 x fovH x fovW floats, 3.0 MB at 16 MP -- from src_rank;
 * the fine levels F-2 .. 0 of THIS rank's window (off_x, off_y) into d_stack (ugsm_submit_fovea_fine).  No event, no second stream,
 * no host synchronisation: stream order is the whole protocol, and the call returns after enqueueing (ugsm_wait / ugsm_poll as usual).
 * Every rank must make the same sequence of shard calls on the same slot numbers (collectives match by order).  With the centre window
 * the result equals ugsm_submit_foveated's, bit for bit.  The reference has one centred fovea on one GPU (MatchGPULib.cpp:1173-1176),
 * seeded from level F-1 (:1230-1240, :1283-1293); the window offset and the shard are this build's (BASELINE.json north_star).
 * librccl.so.1 is loaded on first use (dlopen: a host that never shards does not pay for a 570 MB library); UGSM_ERR_NO_DEVICE when it
 * cannot be found, UGSM_ERR_DEVICE + ugsm_last_error for RCCL failures.
 *
 * WHEN A RANK FAILS (ABI 6).  A collective is a promise to the other ranks, so the library keeps it whatever happens locally:
 *   - what every rank refuses alike (bad arguments, bad geometry, a context whose queue is busy) is refused BEFORE anything is enqueued, on
 *     every rank, and no collective goes out;
 *   - a rank whose pyramids or coarse phase fail afterwards (UGSM_ERR_NOMEM, UGSM_ERR_DEVICE) STILL takes part in the broadcast, then returns
 *     its status from ugsm_submit_fovea_shard.  The state the source sends carries a status word: where the source failed, every other rank's
 *     ugsm_wait / ugsm_poll on that slot answers UGSM_ERR_PEER (ugsm_last_error names the rank and its status; d_stack is not valid).  A
 *     non-source rank that fails harms nobody: the others' results are valid.  The communicator stays usable: the next step runs;
 *   - a rank that never reaches the exchange (a crashed process; a rank that could not even allocate the 3 MB state buffer) cannot be told
 *     from a slow one, so there is a deadline: ugsm_shard_set_timeout(ctx, ms).  A step still unfinished `ms` after its submission makes
 *     ugsm_wait abort the communicator (ncclCommAbort), and answer UGSM_ERR_PEER; every later shard call answers UGSM_ERR_STATE until the host
 *     has called ugsm_shard_finalize and ugsm_shard_init again (on every surviving rank, with a new id).  0 (default): no deadline.
 * ugsm_shard_gather is a collective like the others: after a failed step every rank still makes the gather call its protocol has. */
#define UGSM_SHARD_ID_BYTES 128  /* sizeof(ncclUniqueId) */
/* Rank 0 makes an id (ncclGetUniqueId) and hands its 128 bytes to the other ranks by whatever means the host has (a ROS parameter, a
 * file, MPI, torch.distributed's store): out-of-band, once. */
int ugsm_shard_unique_id(void *id128);
/* One process per GPU: joins the communicator `id128` names as rank `rank` of `world` (ncclCommInitRank).  Collective: returns when
 * all ranks have joined.  A context belongs to at most one communicator (UGSM_ERR_STATE otherwise). */
int ugsm_shard_init(ugsm_ctx *ctx, const void *id128, int rank, int world);
/* One process that owns several GPUs: ctxs[0 .. n) (each created on its own device) become ranks 0 .. n-1 of one communicator
 * (ncclCommInitAll).  The shard calls of the n contexts must then come from ONE HOST THREAD PER CONTEXT (a collective waits for its
 * peers; the library cannot wrap a step in ncclGroupStart / ncclGroupEnd because a grouped broadcast is only launched at the group's
 * end, i.e. after the fine phase that must follow it on the stream). */
int ugsm_shard_init_all(ugsm_ctx *const *ctxs, int n);
int ugsm_shard_rank(const ugsm_ctx *ctx, int *rank, int *world);
/* Number of ranks RCCL itself counts: an ncclAllReduce(sum) of one 1 per rank on slot 0's stream, waited for.  = world when the
 * communicator really spans that many ranks. */
int ugsm_shard_count_ranks(ugsm_ctx *ctx, int *ranks);
int ugsm_submit_fovea_shard(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int off_x,
                            int off_y, float *d_stack, int src_rank);
/* Deadline of a shard step, in milliseconds from its submission (0 = none); see "when a rank fails" above. */
int ugsm_shard_set_timeout(ugsm_ctx *ctx, long long milliseconds);
/* Optional: every rank's fovea stack (3 x (F fovH) x fovW floats, 21 MB at 16 MP) to the one consumer rank -- ncclSend on the others,
 * ncclRecv x (world - 1) + one device copy on dst_rank, on the slot's stream (ordered after the slot's shard call).  d_all (dst_rank
 * only, else NULL): world x stack_floats. */
int ugsm_shard_gather(ugsm_ctx *ctx, int slot, const float *d_stack, long long stack_floats, float *d_all, int dst_rank);
/* Leaves the communicator (ncclCommDestroy); ugsm_destroy does it too. */
int ugsm_shard_finalize(ugsm_ctx *ctx);

/* ---- next row: triangulation of the full-resolution disparity ---------- */

/* CdynamicCalibration::get3DPoint, non-foveated branch (src/pointcloud/getPointCloud.cpp:886-949),
 * for every pixel of the match result instead of the node's scalar host loops (:640-660, :778).
 * d_dispx/d_dispy: H*W device planes (e.g. planes 0 and 1 of ugsm_submit_full's d_out); P1, P2:
 * the 3x4 projection matrices of calL.xml/calR.xml, row-major doubles on the HOST; d_xyz: 3 device
 * planes X, Y, Z.  Enqueued on `slot`'s stream (ordered after a submit on the same slot). */
int ugsm_triangulate(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, int W, int H,
                     const double *P1, const double *P2, float *d_xyz);

/* Row f-1, foveated branch.  Where level `src_level` of the fovea stack sits in level `dest_level` of the
 * full pyramid and the coordinate scale between them: CdynamicCalibration::left_marginOf_in /
 * upper_marginOf_in / mapXcoord (src/pointcloud/getPointCloud.cpp:387-484).  Host only. */
int ugsm_fovea_mapping(int W, int H, int src_level, int dest_level, int *left_margin, int *upper_margin,
                       float *scale);
/* get3DPoint with foveated == 1 (getPointCloud.cpp:892-903) for every pixel of level `src_level` of the
 * (F*fovH) x fovW device stacks d_stackx / d_stacky (the layout ugsm_match_foveated returns);
 * d_xyz: X, Y, Z planes of fovH x fovW floats.  Asynchronous on `slot`, like ugsm_triangulate. */
int ugsm_triangulate_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, int fovW,
                           int fovH, int src_level, int left_margin, int upper_margin, float scale,
                           const double *P1, const double *P2, float *d_xyz);

/* Row f-1, the cloud itself: what the node's doReconstructionRGB / doReconstructionRGB_FOV (src/pointcloud/getPointCloud.cpp:675-722,
 * :615-673) build on the host with one pcl::PointXYZRGB push_back per pixel, built on the device from the planes and the left image.
 * Order as the reference's: column ii outer, row jj inner (a COLUMN-major cloud from row-major planes), pixel (ii, jj) sampled when
 * ii % sampling == 0 && jj % sampling == 0; an unorganised cloud (width = count, height = 1).  X, Y, Z are bit for bit what
 * ugsm_triangulate[_fovea] writes for the pixel; rgb = R << 16 | G << 8 | B of the left image (byte0 << 16 | byte1 << 8 | byte2 of
 * the rgb8 buffer; in another input format, of the pixel's conversion to rgb8: the node's BGR8 copy passes as it is, with
 * UGSM_INPUT_BGR8), alpha 0. */
#define UGSM_CLOUD_PCL32    0  /* pcl::PointXYZRGB as it lies in memory: x, y, z at 0/4/8, 1.0f at 12, the rgb word at 16, 12 zero bytes; point_step 32 */
#define UGSM_CLOUD_XYZRGB16 1  /* x, y, z, rgb at 0/4/8/12; point_step 16 (a PointCloud2 with the same four fields) */
typedef struct ugsm_cloud_params {
    int sampling;        /* >= 1; getPointCloud.cpp:489 uses 1 */
    int format;          /* UGSM_CLOUD_* */
    int compact;         /* 0: every sampled pixel in the reference's order; nonzero: only the kept points, in the same relative order */
    float min_conf;      /* compact: keep conf >= min_conf (a NaN conf is dropped); -inf with d_conf NULL: no confidence test */
    float z_min, z_max;  /* compact: keep z_min <= Z <= z_max; a non-finite X, Y or Z is never kept */
} ugsm_cloud_params;
/* sampling 1, UGSM_CLOUD_PCL32, compact 0, min_conf -inf, z_min -inf, z_max +inf */
void ugsm_default_cloud_params(ugsm_cloud_params *p);
/* points of the dense cloud: ceil(W / sampling) * ceil(H / sampling); -1 on bad arguments.  Host only. */
long long ugsm_cloud_points(int W, int H, int sampling);
/* The cloud of the full-resolution match.  d_dispx / d_dispy / d_conf: H*W device planes (planes 0, 1, 2 of ugsm_submit_full's d_out;
 * d_conf may be NULL when p->min_conf is -inf); d_rgbL: the left image, rgb8 (or the input format), `stride` bytes per row, on the device; P1, P2 as for
 * ugsm_triangulate (host).  d_points (device, 16-byte aligned) receives the first min(count, cap_points) records and nothing past them;
 * *d_count (device) the cloud's number of points, even where that exceeds cap_points.  Asynchronous on `slot`'s stream, like
 * ugsm_triangulate (ordered after a submit on the same slot).  A compact cloud uses a per-slot count buffer that grows on demand
 * (ugsm_context_device_bytes counts it; UGSM_ERR_NOMEM if it cannot grow) and takes two launches; the output is the same byte for byte
 * from run to run.  UGSM_ERR_BAD_ARG: a null pointer, W or H < 1, stride < bytes per pixel * W, sampling < 1, an unknown format, a NaN min_conf / z_min /
 * z_max or z_min > z_max, d_conf NULL with min_conf above -inf, cap_points < 0, a misaligned d_points / d_count, above 2^28 pixels. */
int ugsm_point_cloud(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf,
                     const uint8_t *d_rgbL, int W, int H, int stride, const double *P1, const double *P2,
                     const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count);
/* The foveated form: the points of level src_level of the (F*fovH) x fovW stacks (d_stackc may be NULL as d_conf above), mapped
 * into the full-resolution frame with left_margin / upper_margin / scale (ugsm_fovea_mapping), as ugsm_triangulate_fovea does; the
 * colour is read from the W x H left image at ((int)x1, (int)y1) of the mapped pixel, clamped to the image (at destination level 0
 * no fovea level leaves the image at 16 MP, 1080p, 640 x 480 or 160 x 120; the reference would read outside it where one did). */
int ugsm_point_cloud_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc,
                           int fovW, int fovH, int src_level, int left_margin, int upper_margin, float scale,
                           const uint8_t *d_rgbL, int W, int H, int stride, const double *P1, const double *P2,
                           const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count);

/* The whole fovea stack as ONE cloud (this build's; the reference builds one level at a time).
 *
 * ugsm_fovea_level_mapping is ugsm_fovea_mapping(.., src_level, 0, ..) for any fovea_levels F and for this build's window offsets
 * (off_x, off_y as given to the match).  With w[], h[] of ugsm_level_dims and k = src_level, 0 <= k < F:
 *   scale = powf((float)1.41421356237309504880, (float)k);
 *   left_margin = w[0]/2 - w[F-1-k]/2 + (int)lrint(ex[k] * pow(1.41421356, k)), ex[k] the window's clamped offset from the centre at
 *   level k (0 at level F-1); upper_margin the same with h, ey and off_y.
 * For F == 7 and offset (0, 0) the three equal ugsm_fovea_mapping(W, H, k, 0, ..) exactly.  Host only.  UGSM_ERR_BAD_ARG: a null
 * output, F < 2, F > levels, k outside 0 .. F-1, a size ugsm_level_dims refuses for the stack's
 * F levels (the levels below the stack do not enter).
 *
 * THE COVERAGE RULE.  Pixel (ii, jj) of level k >= 1 has the footprint [x1, x1 + scale_k) x [y1, y1 + scale_k) in the full-resolution
 * frame, x1 = (float)left_k + (float)ii * scale_k and y1 = (float)upper_k + (float)jj * scale_k (the cloud's own x1, y1).  It is COVERED,
 * and left out of the merged cloud, when that footprint lies wholly inside level k-1's window:
 *   x1 >= (float)left_{k-1} && x1 + scale_k <= (float)left_{k-1} + (float)fovW * scale_{k-1}, and the same in y with upper and fovH,
 * every operation in binary32 and rounded on its own.  Level 0 covers nothing.  A pixel that straddles a window's edge is kept: the
 * cloud has a one-pixel seam of overlap and never a hole.  Per level the covered columns are one interval and the covered rows another.
 *
 * ugsm_fovea_cloud_points: the dense size of the merged cloud -- per level (sampled columns) x (sampled rows) less (sampled covered
 * columns) x (sampled covered rows), written to per_level[0 .. F-1] when that is not NULL -- or -1 on bad arguments.  Host only.
 * 16 MP, 14 / 7 levels, centred: 1 005 221 points of the stack's 1 752 135.
 *
 * ugsm_point_cloud_fovea_all: levels and fovea_levels are the context's; d_stackx / d_stacky / d_stackc the (F*fovH) x fovW stacks of a
 * foveated call, off_x / off_y as given to it.  Level 0 comes first, then 1 .. F-1; within a level the order is ugsm_point_cloud_fovea's
 * (column outer, row inner, the sampled pixels) with the covered pixels left out.  Each record is byte for byte the one
 * ugsm_point_cloud_fovea writes for that pixel with ugsm_fovea_level_mapping's numbers for its level, in either record format and
 * any input format.  Dense: every uncovered sampled pixel, *d_count = ugsm_fovea_cloud_points(..).  Compact: the kept points only (the
 * same test), in the same relative order, the same bytes from run to run.  cap_points, *d_count, the stream and the count buffer as for
 * ugsm_point_cloud.  d_level_counts (device, 8-byte aligned, F entries; may be NULL) receives each level's number of points in the
 * cloud, so that a consumer knows where each resolution starts.  One launch (compact: two) for the whole stack.
 * UGSM_ERR_BAD_ARG as for ugsm_point_cloud_fovea, and also: a context with fovea_levels < 2 (a one-level stack is the full frame:
 * ugsm_point_cloud), a misaligned d_level_counts. */
int ugsm_fovea_level_mapping(int W, int H, int levels, int fovea_levels, int off_x, int off_y, int src_level,
                             int *left_margin, int *upper_margin, float *scale);
long long ugsm_fovea_cloud_points(int W, int H, int levels, int fovea_levels, int off_x, int off_y, int sampling,
                                  long long *per_level);
int ugsm_point_cloud_fovea_all(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc,
                               int W, int H, int off_x, int off_y, const uint8_t *d_rgbL, int stride,
                               const double *P1, const double *P2, const ugsm_cloud_params *p, void *d_points,
                               long long cap_points, long long *d_count, long long *d_level_counts);

/* The stacks of SEVERAL WINDOWS of one pair as ONE cloud (this build's): what follows ugsm_submit_foveated_multi as
 * ugsm_point_cloud_fovea_all follows ugsm_submit_foveated.
 *
 * Inputs: n stacks, 1 <= n <= UGSM_MAX_BATCH, each laid out as ugsm_submit_foveated_multi writes it -- 3 x (F*fovH) x fovW, planes dx, dy,
 * conf -- and the off_x[j], off_y[j] given to that call (NULL = all centred).  left[j][k], upper[j][k], scale_k: ugsm_fovea_level_mapping's
 * numbers for level k and window j's offset; at k = F-1 the margins are 0 for every window.
 *
 * ENTRIES.  The cloud is a sequence of E = (F-1)*n + 1 entries, level-major: entry e = k*n + j is level k of window j for k = 0 .. F-2 and
 * j = 0 .. n-1; the last entry e = (F-1)*n is the whole-frame level F-1, read from stack 0 alone (row block F-1 is the same field in every
 * stack by the matching contract, so it is emitted once).  Within an entry the order is ugsm_point_cloud_fovea's (the sampled pixels,
 * column outer, row inner), and each record is byte for byte the one ugsm_point_cloud_fovea writes for that pixel of that stack with the
 * entry's mapping, in either record format and any input format.
 *
 * THE RULE ACROSS WINDOWS.  Pixel (ii, jj) of entry (j, k) lies at x1 = (float)left[j][k] + (float)ii * scale_k,
 * y1 = (float)upper[j][k] + (float)jj * scale_k (the cloud's own x1, y1).  inside(i, m) holds when
 *   x1 >= (float)left[i][m] && x1 + scale_k <= (float)left[i][m] + (float)fovW * scale_m, and the same in y with upper and fovH,
 * every operation in binary32 and rounded on its own.  The pixel is LEFT OUT when
 *   (a) k >= 1 and inside(i, k-1) for some window i in 0 .. n-1, its own included: a finer level of any window covers it; or
 *   (b) k <= F-2 and inside(i, k) for some i > j: the same level of a higher-numbered window holds it (the highest index wins, as in
 *       ugsm_reconstruct_full_multi).
 * A pixel that straddles an edge is kept: the cloud has seams of overlap and never a hole.  (b) is stated in the mapped frame, not on the
 * level's integer grid: left[j][k] rounds each window's offset on its own, and the integer-grid form leaves slivers uncovered.  With
 * n == 1, (b) is empty and (a) is the coverage rule above: the call is byte for byte ugsm_point_cloud_fovea_all, the count and the
 * per-level counts included.  Per entry the left-out set is a union of at most 2n-1 rectangles of the sampled grid.
 *
 * ugsm_fovea_multi_cloud_points: the dense size of the merged cloud; per_entry (may be NULL) receives the E entry sizes; -1 on bad
 * arguments.  Host only.
 *
 * ugsm_point_cloud_fovea_multi: levels and fovea_levels are the context's.  d_stack is a HOST array of n DEVICE stacks, as
 * ugsm_reconstruct_full_multi takes it; a stack's confidence plane is its third plane, read only by a compact cloud with min_conf above
 * -inf.  Dense: every sampled pixel the rule keeps, *d_count = ugsm_fovea_multi_cloud_points(..).  Compact: the ugsm_cloud_params test
 * applied after the rule, the relative order kept, the same bytes from run to run.  cap_points, *d_count and the count buffer as for
 * ugsm_point_cloud_fovea_all (the buffer grows on demand, counted by ugsm_context_device_bytes; UGSM_ERR_NOMEM if it cannot).
 * d_entry_counts (device, 8-byte aligned, E entries; may be NULL) receives each entry's number of points in the cloud.  One launch
 * (compact: two) for all entries.  Asynchronous on `slot`'s stream -- so ordered behind a ugsm_submit_foveated_multi on the same slot --
 * and the call itself does not wait for the stream unless one of its buffers has to grow.
 * UGSM_ERR_BAD_ARG, before any device work: everything ugsm_point_cloud_fovea_all refuses, n outside 1 .. UGSM_MAX_BATCH, a null array or
 * entry, a misaligned d_entry_counts.  UGSM_ERR_STATE: pairs enqueued with ugsm_enqueue_* are outstanding.
 * The stacks of ugsm_submit_foveated_multi_checked go in as any others: a compact cloud with min_conf > 0 leaves the marked pixels out.
 * NOT built: a queue or managed form of this call; the resized cloud of several stacks; the ros/ shim does not call it. */
long long ugsm_fovea_multi_cloud_points(int W, int H, int levels, int fovea_levels, int n, const int *off_x, const int *off_y,
                                        int sampling, long long *per_entry);
int ugsm_point_cloud_fovea_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H,
                                 const int *off_x, const int *off_y, const uint8_t *d_rgbL, int stride,
                                 const double *P1, const double *P2, const ugsm_cloud_params *p, void *d_points,
                                 long long cap_points, long long *d_count, long long *d_entry_counts);

/* Row f-1, the resized cloud: what the node publishes on output_pointcloud_resized, doReconstruction_resized /
 * doReconstructionFOV_resized (getPointCloud.cpp:724-800, :802-884).  The Z plane resized with cv::resize(..., INTER_CUBIC) to
 * dw x dh = (int)((float)pw * factor) x (int)((float)ph * factor) (pw x ph: W x H, or fovW x fovH), then one point per pixel (ii, jj)
 * of the resized map, column ii outer and row jj inner: X, Y are ugsm_triangulate[_fovea]'s at xx = (int)((float)ii / factor),
 * yy = (int)((float)jj / factor) (IEEE float division), Z the resized map's (ii, jj), the colour the left image's at (xx, yy).
 * The reference's registration is kept: X, Y sit at (int)(ii / f) while the cubic's centre lies near ii / f + (1 / f - 1) / 2.
 * INTER_CUBIC on CV_32F is OpenCV's generic path (resizeGeneric_, HResizeCubic / VResizeCubic), restated in float:
 *   scale = 1. / ((double)dw / pw); fx = (float)((dx + 0.5) * scale - 0.5); sx = floor(fx); fx -= sx  (rows the same with dy);
 *   A = -0.75f; c0 = ((A*(x+1) - 5*A)*(x+1) + 8*A)*(x+1) - 4*A, c1 = ((A+2)*x - (A+3))*x*x + 1,
 *   c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1, c3 = 1.f - c0 - c1 - c2;
 *   taps sx-1 .. sx+2 and sy-1 .. sy+2 clamped to the plane; each source row S[sx-1]*c0 + S[sx]*c1 + S[sx+1]*c2 + S[sx+2]*c3 left to
 *   right, from +0.0f on the columns with sx < 1 or sx + 2 >= pw; then ((R0*b0 + R1*b1) + R2*b2) + R3*b3; no fused multiply-add;
 *   NaN and inf propagate (a zero coefficient times inf is NaN).  When the size does not change (factor 1) cv::resize copies, and Z
 *   is the pixel's own.  Builds of OpenCV that take IPP or a fused vertical pass may differ in the last bit.
 * Otherwise as ugsm_point_cloud[_fovea]: asynchronous on `slot`'s stream, the same records, cap_points and *d_count, and compaction
 * (finite X, Y and resized Z, z_min <= Z <= z_max, conf(xx, yy) >= min_conf).  UGSM_ERR_BAD_ARG as there, and also: p->sampling other
 * than 1 (the resized cloud has none), a factor that is not finite and in (0, 1] or leaves a side 0, colour_mapped not 0 or 1. */
/* points of the resized cloud: (int)((float)W * factor) * (int)((float)H * factor); -1 when factor is not in (0, 1] or a side truncates to 0 */
long long ugsm_resized_cloud_points(int W, int H, float factor);
int ugsm_point_cloud_resized(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf,
                             const uint8_t *d_rgbL, int W, int H, int stride, const double *P1, const double *P2, float factor,
                             const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count);
/* The foveated form, on level src_level of the stacks.  colour_mapped 0: the colour at (xx, yy) of the W x H image, unmapped -- the
 * reference's own reading (:864-867), from the image's top-left corner; 1: at the mapped pixel, as ugsm_point_cloud_fovea reads it.
 * Either is clamped to the image. */
int ugsm_point_cloud_resized_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc,
                                   int fovW, int fovH, int src_level, int left_margin, int upper_margin, float scale,
                                   const uint8_t *d_rgbL, int W, int H, int stride, const double *P1, const double *P2, float factor,
                                   int colour_mapped, const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count);

/* ---- row f-1, the depth image: REP 118 32FC1 / 16UC1 ----------------------------------------------------------------------------------
 *
 * The one intermediate the reference's point-cloud node builds explicitly: doReconstruction_resized / doReconstructionFOV_resized fill a
 * range_map with the Z of get3DPoint, pixel for pixel and row-major, and cv::resize it to res_range_map (getPointCloud.cpp:730-758,
 * :813-841, :951-1021).  These calls hand that map out as the depth image REP 118 defines, registered to the left camera: row-major and
 * contiguous, dw x dh elements of 4 or 2 bytes -- the payload of a sensor_msgs/Image with step = dw * size.
 *
 * Per pixel, in this order, every operation in binary32 and rounded on its own:
 *   Z      factor == 1: the image is pw x ph (W x H; the fovea form: fovW x fovH) and Z is bit for bit the Z that ugsm_triangulate
 *          (ugsm_triangulate_fovea with ugsm_fovea_level_mapping's numbers) writes for the pixel.  factor < 1: the image is dw x dh =
 *          (int)((float)pw * factor) x (int)((float)ph * factor), ugsm_depth_image_size, and Z of (ii, jj) is bit for bit the z of record
 *          (ii, jj) of ugsm_point_cloud_resized[_fovea] -- the same taps, coefficients, sum order and border rule, the same copy at an
 *          unchanged size; the confidence is read at (xx, yy), xx = (int)((float)ii / factor), yy = (int)((float)jj / factor), as there.
 *   valid  Z finite, z_min <= Z <= z_max, and (d_conf NULL or conf >= min_conf; a NaN confidence fails).  X and Y play no part.
 *   32F    m = Z * unit; stored where valid, else the quiet NaN 0x7FC00000.  With the default parameters every finite Z is stored as it is.
 *   16U    u = (m * 1000.0f) + 0.5f; valid additionally requires u >= 1.0f && u < 65536.0f; (uint16_t)u (truncation) where valid, else 0.
 * *d_valid (device, 8-byte aligned, may be NULL) receives the number of valid pixels stored; the call zeroes it on the slot's stream.  It is
 * a sum of integers (ballots and popcounts, one integer atomic per workgroup), the same from run to run.
 *
 * unit: metres per unit of Z, that is, of the calibration's translation (P2[0][3] / P2[0][0] is the baseline in that unit).
 *
 * Memory: d_depth (device) need only be aligned to its element, the planes to 4 bytes (plane 1 of a d_out starts at 4 W H bytes); nothing is
 * written outside [d_depth, d_depth + images * dw * dh * size).  d_depth must not overlap d_dispx / d_dispy / d_conf (the stacks).
 *
 * ugsm_depth_image_fovea: d_stackx / d_stacky / d_stackc are the (F*fovH) x fovW stacks of a foveated call on a W x H frame with the
 * window offset (off_x, off_y); levels and fovea_levels are the context's, each level mapped with ugsm_fovea_level_mapping.  level in
 * 0 .. F-1: that level's image.  UGSM_DEPTH_ALL_LEVELS: every level in ONE launch, the images laid out as stackH is -- (F * dh) x dw,
 * level 0 first -- and d_valid holds F counts.  A fovea level converts xx + disparity with (int), as the reference does: for a NaN
 * disparity or one beyond the range of int that conversion is undefined, as it is for ugsm_triangulate_fovea and the fovea clouds.
 *
 * ugsm_match_full_depth: the blocking call, ugsm_match_full followed by ugsm_depth_image on the same slot (slot 0).  `depth` (host memory
 * of any kind) receives the image; each of dispH / dispV / dispC may be NULL and is then not downloaded: with all three NULL only the depth
 * image crosses the bus.  d_conf is the match's confidence plane.  The images are read in the context's input format.
 *
 * ugsm_depth_image[_fovea] are asynchronous on `slot`'s stream, like ugsm_triangulate -- so ordered behind a ugsm_submit_* on the same
 * slot -- and make no host synchronisation.  UGSM_ERR_STATE: pairs enqueued with ugsm_enqueue_* are outstanding.  UGSM_ERR_BAD_ARG, before
 * any device work: a null pointer (d_conf / d_stackc / d_valid excepted); d_conf NULL with min_conf above -inf; an unknown format; a unit
 * that is not finite and > 0; a NaN min_conf / z_min / z_max, or z_min > z_max; a factor that is not finite and in (0, 1] or leaves a side
 * 0; W or H < 1, or more than 2^28 pixels; a misaligned d_depth / d_valid / plane; d_depth overlapping an input; a bad slot or level; the
 * fovea form on a context with fovea_levels < 2.
 *
 * THE WHOLE FRAME FROM A FOVEA STACK -- ugsm_depth_image_fovea_full, ugsm_depth_image_fovea_multi, ugsm_match_foveated_depth.  One W x H (or
 * resized) image registered to the left camera from the stack of a foveated call (_multi: from the n stacks of
 * ugsm_submit_foveated_multi[_checked]).  The contract is one sentence: the image and *d_valid are byte for byte what
 * ugsm_reconstruct_full (_multi: ugsm_reconstruct_full_multi) into a 3 W H field, followed by ugsm_depth_image on that field's three planes
 * with the same P1, P2, p and the same lens setting, would give.  The full-resolution field is never formed: one launch (and the zeroing of
 * *d_valid), no level buffers, no slot memory beyond a table of n > 1 windows.  What the sentence implies:
 *   value     of frame pixel (x, y): descend from level 0.  At level l < F-1 the site is inside the window when 0 <= x - ox[l] < fovW &&
 *             0 <= y - oy[l] < fovH, ox / oy the window's origin at level l as the foveated call places it (off_x, off_y clamped to the
 *             level).  _multi: every window is tested and the HIGHEST-numbered window that holds the site supplies the value.  Otherwise
 *             move to x = tex(((float)x + 0.5f) / s, w[l+1]), the same in y (s = (float)1.41421356; tex: floor, clamped to 0 .. n-1).
 *             Level F-1 holds every site; _multi reads it from stack 0.
 *   scaling   the three values read (dx, dy, conf) are multiplied by s once per level descended, each product rounded on its own -- the
 *             confidence too, as hierarchicalDisparity scales every channel: min_conf tests conf * s^depth, as it does in the composition.
 *   Z         the FIELD form, not the fovea form: x1 = x, y1 = y, x2 = x + dx, y2 = y + dy, no (int) conversion and no level mapping; then
 *             the lens if one is set and the rule above, exactly as ugsm_depth_image applies them.  A disparity never indexes memory, so NaN,
 *             infinite and huge values are defined here, unlike in the per-level fovea form.
 *   factor    < 1: the image is ugsm_depth_image_size(W, H, factor), Z the resized clouds' cubic resize of the 16 footprint Z, each from
 *             its own descent, the confidence read by descent at (xx, yy) = ((int)((float)ii / factor), (int)((float)jj / factor)).
 * d_stackc NULL (with min_conf -inf): no confidence test, as ugsm_depth_image with d_conf NULL; _multi takes each stack as 3 planes of F
 * levels (d_stack: a HOST array of n DEVICE stacks; off_x / off_y NULL = centred) and always tests the confidence (a NaN fails).
 * Both are asynchronous on `slot`, ordered behind a ugsm_submit_foveated* on the same slot, and make no host synchronisation (the table of
 * n > 1 windows goes up on the slot's stream; only its first growth waits for the stream).  Refused before any device work, nothing written,
 * ugsm_last_error naming the call: everything ugsm_depth_image refuses (the planes being the stacks); fovea_levels < 2; n outside
 * 1 .. UGSM_MAX_BATCH or a null stack entry; d_depth overlapping any stack; UGSM_ERR_STATE while pairs enqueued with ugsm_enqueue_* are
 * outstanding.  ugsm_match_foveated_depth: the blocking call, ugsm_match_foveated followed by ugsm_depth_image_fovea_full on slot 0; each of
 * stackH / stackV / stackC may be NULL and is then not downloaded (the sibling of ugsm_match_full_depth).
 *
 * Out of scope: queue forms (ugsm_enqueue_*_depth*), also of the whole-frame image; the whole frame's X, Y, Z planes or cloud without the
 * field (compose ugsm_reconstruct_full[_multi] with ugsm_triangulate / ugsm_point_cloud); a strided output; depth in the right camera;
 * camera_info handling
 * (a host hands K and D over with ugsm_set_lens, "lens distortion" below); undistortion of the image itself (the lens setting undistorts the
 * two positions of each correspondence, the image's grid stays the distorted left camera's). */
#define UGSM_DEPTH_32F 0   /* REP 118 32FC1: float, NaN where there is no reading */
#define UGSM_DEPTH_16U 1   /* REP 118 16UC1: uint16 millimetres, 0 where there is no reading */
#define UGSM_DEPTH_ALL_LEVELS (-1)
typedef struct ugsm_depth_params {
    int   format;        /* UGSM_DEPTH_* */
    float unit;          /* metres per unit of Z (the calibration's unit); > 0, finite */
    float min_conf;      /* keep conf >= min_conf; -inf with d_conf NULL: no confidence test (the clouds' rule) */
    float z_min, z_max;  /* keep z_min <= Z <= z_max, on Z itself (before unit) */
    float factor;        /* 1.0f: the range map itself; in (0, 1): the reference's res_range_map */
} ugsm_depth_params;
/* UGSM_DEPTH_32F, unit 1.0f, min_conf -inf, z_min -inf, z_max +inf, factor 1.0f */
void ugsm_default_depth_params(ugsm_depth_params *p);
/* the image's size, the resized clouds' rule: (int)((float)pw * factor) x (int)((float)ph * factor).  Host only.  UGSM_ERR_BAD_ARG: a null
 * output, pw or ph < 1, a factor that is not in (0, 1] or leaves a side 0. */
int ugsm_depth_image_size(int pw, int ph, float factor, int *dw, int *dh);
int ugsm_depth_image(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf, int W, int H,
                     const double *P1, const double *P2, const ugsm_depth_params *p, void *d_depth,
                     unsigned long long *d_valid);
int ugsm_depth_image_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc,
                           int W, int H, int off_x, int off_y, int level, const double *P1, const double *P2,
                           const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid);
int ugsm_match_full_depth(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                          const double *P1, const double *P2, const ugsm_depth_params *p, void *depth, float *dispH,
                          float *dispV, float *dispC);
/* one W x H (or resized) depth image registered to the left camera, from the stack of a foveated call */
int ugsm_depth_image_fovea_full(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc,
                                int W, int H, int off_x, int off_y, const double *P1, const double *P2,
                                const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid);
/* the same from the n stacks of ugsm_submit_foveated_multi[_checked] (HOST array of n DEVICE stacks, 3 planes of F levels each;
 * off_x / off_y NULL = centred) */
int ugsm_depth_image_fovea_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H,
                                 const int *off_x, const int *off_y, const double *P1, const double *P2,
                                 const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid);
/* blocking: ugsm_match_foveated, then ugsm_depth_image_fovea_full on slot 0; each of stackH / stackV / stackC may be NULL and is then
 * not downloaded (the sibling of ugsm_match_full_depth) */
int ugsm_match_foveated_depth(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                              const double *P1, const double *P2, const ugsm_depth_params *p, void *depth,
                              float *stackH, float *stackV, float *stackC);

/* ---- lens distortion: plumb_bob D in triangulation, clouds and depth -----------------------------------------------------------------
 *
 * Every 3-D output above comes from one closed form that takes the two pixel positions (x1, y1), (x2, y2) of a correspondence as ideal
 * pinhole coordinates under P1 and P2.  With a lens set, (x1, y1) is undistorted by camera 1's K1, D1 and (x2, y2) by camera 2's K2, D2 just
 * before the closed form.  Images, match and fields stay as they are; nothing is resampled.  (The reference's cloud node reads K and D from
 * the two CameraInfo messages and never uses them.)
 *
 * The definition, for K (3 x 3 row-major: fx = K[0], fy = K[4], cx = K[2], cy = K[5]; skew ignored), D = (k1, k2, p1, p2, k3) and a pixel
 * coordinate (u, v) held as binary32; every operation binary64 and rounded on its own, division IEEE:
 *     x0 = ((double)u - cx) / fx;   y0 = ((double)v - cy) / fy;   x = x0; y = y0;
 *     `iterations` times:
 *         r2 = x*x + y*y;
 *         ic = 1.0 / (1.0 + ((k3*r2 + k2)*r2 + k1)*r2);
 *         dX = 2.0*p1*x*y + p2*(r2 + 2.0*x*x);
 *         dY = p1*(r2 + 2.0*y*y) + 2.0*p2*x*y;
 *         x = (x0 - dX)*ic;   y = (y0 - dY)*ic;
 *     u' = (float)(x*fx + cx);   v' = (float)(y*fy + cy);
 * -- the fixed-point iteration of OpenCV's undistortPoints with R = I, P = K, restated (not pinned against OpenCV).  With all five
 * coefficients zero, u' and v' are u and v bit for bit for every coordinate in and around a frame (the binary64 round trip errs by about
 * 1e-12 px); zero D is not special-cased, and a zero-D lens gives the bytes of no lens.
 *
 * Everything else about a point is unchanged: the colour is read at the original pixel; the fovea forms map first and undistort the mapped
 * positions, and keep (int)x1 of the mapped, distorted x1; the coverage rule of ugsm_point_cloud_fovea_all is a rule about pixels and stays
 * on the mapped, distorted positions; a compact cloud tests the X, Y, Z that result; record formats, order and counts, and the 16UC1
 * rounding, are as without a lens.
 *
 * ugsm_set_lens: four host arrays (9, 5, 9, 5 doubles) as sensor_msgs/CameraInfo holds them; iterations 1 .. 32, 0 = 5 (OpenCV's count).
 * All four arrays NULL switches the lens off, the state of a new context.  It is a setting, read when a call is made, as
 * ugsm_set_input_format: the values travel in the launch's arguments, so a change between two calls enqueued on one slot does not reach the
 * earlier one.  UGSM_ERR_BAD_ARG -- the setting stays as it was -- for some but not all arrays NULL, a non-finite entry, !(fx > 0) or
 * !(fy > 0), iterations outside 0 .. 32.
 * ugsm_get_lens: *set = 1 and the values (any output but `set` may be NULL) while a lens is set, else *set = 0 and nothing else written.
 * ugsm_undistort_points: the definition on the host for n points, uv_in / uv_out n pairs (u, v) (they may be the same array); needs no
 * context and no device.  UGSM_ERR_BAD_ARG for a NULL K or D, n < 0, NULL points with n > 0, and the value checks of ugsm_set_lens.
 *
 * Honoured by: ugsm_triangulate, ugsm_triangulate_fovea, ugsm_point_cloud, ugsm_point_cloud_fovea, ugsm_point_cloud_fovea_all,
 * ugsm_point_cloud_resized and ugsm_point_cloud_resized_fovea (every one of the 16 footprint Z), ugsm_depth_image and
 * ugsm_depth_image_fovea (both formats, any factor, UGSM_DEPTH_ALL_LEVELS), ugsm_match_full_depth, ugsm_depth_image_fovea_full,
 * ugsm_depth_image_fovea_multi and ugsm_match_foveated_depth.
 * Refused while a lens is set -- UGSM_ERR_STATE, nothing enqueued, nothing written, ugsm_last_error names the setting --:
 * ugsm_point_cloud_fovea_multi and every ugsm_enqueue_*_cloud* (the queue's pair records do not capture the lens yet). */
int ugsm_set_lens(ugsm_ctx *ctx, const double *K1, const double *D1, const double *K2, const double *D2, int iterations);
int ugsm_get_lens(const ugsm_ctx *ctx, double *K1, double *D1, double *K2, double *D2, int *iterations, int *set);
int ugsm_undistort_points(const double *K, const double *D, int iterations, const float *uv_in, float *uv_out, long long n);

/* ---- the cloud from the queue: enqueue a pair, get its cloud back ------------------------------------------------------------------
 *
 * The slot-level cloud calls above answer UGSM_ERR_STATE while enqueued pairs are outstanding, and a managed pair never shows its device
 * planes.  These forms of ugsm_enqueue_* carry the cloud with the pair: the call the pair goes out in runs the match, then the clouds of
 * all its pairs on the same slot stream -- ONE launch for the call (compact: two), the pair an index of the grid, each pair's arguments
 * read from a table in device memory.  (Where the matcher itself goes pair by pair -- calls of one pair, contexts with the full-mode LR
 * check or early exit -- and where one pair's cloud evaluates more than 9 M sampled points, the size above which the matcher's own levels
 * go pair by pair (a 16 MP full-mode cloud at sampling 1), the clouds are launched pair by pair too.)
 *   The full-mode cloud is, byte for byte, what ugsm_point_cloud writes for that pair's planes and left image with the same params, P1,
 * P2 and input format; the foveated cloud what ugsm_point_cloud_fovea_all writes for the pair's stack and its off_x, off_y -- however
 * the queue grouped the pairs.  The colour words follow the input format captured at enqueue; with the LR check on, a compact cloud
 * with min_conf > 0 leaves the marked pixels out, in either mode.
 *   The spec is copied when the pair is enqueued.  Pairs of one call now also share a byte-equal spec (P1, P2, params, want_planes): a
 * pair with another spec, or without a cloud, ends the group exactly as a pair of another kind does.
 *   UGSM_ERR_BAD_ARG, nothing enqueued: everything ugsm_enqueue_full / ugsm_enqueue_foveated and the slot-level cloud calls reject (a null
 * spec, sampling < 1, an unknown format, a NaN min_conf / z_min / z_max or z_min > z_max, cap_points < 0, a misaligned d_points /
 * d_count / d_level_counts), max_points < 0, and the foveated forms on a context with fovea_levels < 2.
 *   Device forms: d_out / d_stack receive the pair's result as with ugsm_enqueue_full / ugsm_enqueue_foveated; d_points, cap_points,
 * *d_count and d_level_counts (may be NULL) behave as in the slot-level calls -- the count may exceed the cap, nothing is written past
 * min(count, cap) records.  Every buffer stays valid and untouched until the pair's tag has been reported.
 *   Managed forms: any host memory in (copied before the call returns), a library-owned page-locked cloud out, fetched with
 * ugsm_done_cloud after the ugsm_next_done that reported the pair.  want_planes 0: the result planes are NOT downloaded -- they stay in
 * the slot's device buffers, where the cloud reads them -- and ugsm_completion.result[] is NULL; nonzero: they are lent as by
 * ugsm_enqueue_*_managed.  The cloud's size is only known on the device, so a managed call completes in two steps: its counts come down
 * with the call; when the library notices the slot idle it reads them and enqueues one device-to-host copy (the copy engine, not a
 * kernel) of stored x point_step bytes per pair on the slot's stream, and the pairs are reported when that has drained.  The slot stays
 * busy in between; order of reporting and "a completion means every buffer of the pair, cloud buffers included, is no longer in use" are
 * unchanged, and a failed call's pairs are reported with the call's status after the slot has drained, as ever.
 *   Memory of the managed forms: per slot, pairs x cap x point_step bytes of device cloud (cap = max_points, or the dense size when that is
 * 0), grown on demand and counted by ugsm_context_device_bytes -- a call that cannot get them is reported with UGSM_ERR_NOMEM; per managed
 * buffer, page-locked staging that grows to the largest `stored` seen, never to the dense size up front (dense PCL32 at 16 MP is 514 MB
 * per pair, and (slots + 1) x batch pairs may be outstanding).
 *   Out of scope: the page-locked _host kind, the resized cloud and the single-level fovea cloud have no queue form. */
typedef struct ugsm_queue_cloud {
    double P1[12], P2[12];     /* as ugsm_point_cloud: row-major 3x4, copied at enqueue */
    ugsm_cloud_params params;  /* sampling, format, compact, min_conf, z_min, z_max */
    long long max_points;      /* managed: cap of the library-owned cloud; 0 = the dense size */
    int want_planes;           /* managed: also lend the result planes through ugsm_completion.result (0: they are not downloaded) */
    int reserved;              /* 0 */
} ugsm_queue_cloud;
int ugsm_enqueue_full_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out,
                            const ugsm_queue_cloud *spec, void *d_points, long long cap_points, long long *d_count, uint64_t tag);
int ugsm_enqueue_foveated_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int off_x, int off_y,
                                float *d_stack, const ugsm_queue_cloud *spec, void *d_points, long long cap_points, long long *d_count,
                                long long *d_level_counts, uint64_t tag);
int ugsm_enqueue_full_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride,
                                    const ugsm_queue_cloud *spec, uint64_t tag);
int ugsm_enqueue_foveated_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x,
                                        int off_y, const ugsm_queue_cloud *spec, uint64_t tag);
typedef struct ugsm_cloud_result {
    void *points;             /* page-locked, point_step bytes per record, valid until the NEXT ugsm_next_done on this context */
    long long count, stored;  /* the cloud's size; records at `points` = min(count, cap) */
    int point_step, levels;   /* 32 or 16; fovea_levels for a foveated pair, else 0 */
    long long level_counts[UGSM_MAX_LEVELS];
} ugsm_cloud_result;
/* The cloud of the pair the last ugsm_next_done reported.  UGSM_ERR_STATE if that pair carried no managed cloud, if its call failed, or if
 * nothing has been reported yet. */
int ugsm_done_cloud(ugsm_ctx *ctx, ugsm_cloud_result *out);

/* ---- checked pairs through the queue: both directions of the pairs of a call in lockstep, each pair with a tau of its own -----------------
 *
 * A plain ugsm_enqueue_full* on a context with ugsm_set_lr_check(ctx, tau, UGSM_LR_FULL) is checked the context's way: its call goes pair by
 * pair, every pair matched a second time with the images exchanged, the right camera's field thrown away, tau one setting for everything
 * outstanding.  These forms carry the check with the pair instead: the call a pair goes out in is ONE ugsm_submit_full_checked[_host] of its
 * pairs -- the pyramids once, 2 n fields in lockstep, one check launch -- and launches nothing that call does not launch.  They neither read
 * nor change ugsm_set_lr_check; plain pairs on the same context behave exactly as before.
 *   The contract, bit for bit: d_out, and d_back where given, of a pair are what ugsm_submit_full_checked writes for that pair alone with that
 * tau (dx and dy the unchecked matches', the confidences zeroed where the check fails), in the input format captured at enqueue, however the
 * queue grouped the pairs; the managed planes are the same fields.  The cloud forms: byte for byte, count included, what ugsm_point_cloud
 * writes for the pair's CHECKED forward planes and left image -- a compact cloud with min_conf > 0 leaves the marked pixels out.
 *   Grouping: pairs of one call are all checked, with one bit-equal tau, or all plain; a pair of another tau, a plain pair, a pair with or
 * without a cloud ends the group as a pair of another kind does.  Pairs of one call may differ in whether they take the right camera's field.
 * Call sizes, the stagger, back-pressure and the (slots + 1) x batch limit are those of every other pair (ugsm_queue_plan).
 *   d_back (device forms): may be NULL -- that pair's right-to-left field then stays in the slot.  want_back (managed forms): nonzero lends the
 * right camera's checked planes too, through ugsm_done_checked; ugsm_completion.result[0 .. 2] are the checked forward planes (NULL for a cloud
 * pair without want_planes), result[3] and result[4] NULL.
 *   Refused with nothing enqueued, after the refusals of ugsm_enqueue_full[_managed] and before those of the cloud spec and of a full queue:
 * !(tau > 0), NaN included: UGSM_ERR_BAD_ARG; a context with early_exit_threshold > 0 or kernel_path 1: UGSM_ERR_BAD_ARG; a runtime without the
 * checked call: UGSM_ERR_STATE.  A call that fails -- UGSM_ERR_NOMEM where the level buffers cannot hold 2 n full fields: sixteen fields for a
 * call of eight, 17 GB at 16 MP -- is reported through each pair's ugsm_completion.status once the slot has drained, as ever.
 *   Memory of the managed forms: per slot, one device field per pair of a call (two for a pair with want_back) of result staging, and the
 * page-locked staging of a pair grows by three planes with want_back.
 *   Out of scope: a page-locked _host kind of these forms; foveated pairs (UGSM_LR_FOVEATED already runs their check in lockstep through the
 * queue); seeded or coarse / fine pairs. */
int ugsm_enqueue_full_checked(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out,
                              float *d_back /* may be NULL */, float tau, uint64_t tag);
int ugsm_enqueue_full_checked_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float tau,
                                      int want_back, uint64_t tag);
int ugsm_enqueue_full_checked_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out,
                                    float *d_back /* may be NULL */, float tau, const ugsm_queue_cloud *spec, void *d_points,
                                    long long cap_points, long long *d_count, uint64_t tag);
int ugsm_enqueue_full_checked_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float tau,
                                            int want_back, const ugsm_queue_cloud *spec, uint64_t tag);
typedef struct ugsm_checked_result {
    float *back[3];                     /* managed with want_back: page-locked H, V, C planes of the right camera's checked field, valid until the
                                           NEXT ugsm_next_done on this context; else NULL */
    long long marked_fwd, marked_back;  /* what ugsm_last_lr_marked_pair answers for the pair */
} ugsm_checked_result;
/* For the pair the last ugsm_next_done reported.  UGSM_ERR_STATE if that was no checked pair, if its call failed, or if nothing has been
 * reported yet. */
int ugsm_done_checked(ugsm_ctx *ctx, ugsm_checked_result *out);

/* Row f-3: MatchGPULib::hierarchicalDisparity (MatchGPULib.cpp:2589-2701, kernel MatchLib.cu:435-462):
 * one full-resolution (dx, dy, conf) field from the foveated stacks -- the coarsest fovea level (the whole
 * frame) upsampled level by level (x SCALE, every channel), each finer fovea pasted at its window.
 * d_stackH/V/C: device, (fovea_levels*fovH) x fovW each; d_out3: device, 3 planes W x H.
 * off_x/off_y as passed to ugsm_match_foveated.  Asynchronous on `slot`; ugsm_wait(ctx, slot) to finish. */
int ugsm_reconstruct_full(ugsm_ctx *ctx, int slot, const float *d_stackH, const float *d_stackV,
                          const float *d_stackC, int W, int H, int off_x, int off_y, float *d_out3);

/* hierarchicalDisparity over the n stacks of ugsm_submit_foveated_multi (HOST array of n DEVICE stacks; off_x / off_y as passed there, NULL =
 * centred): one full-resolution (dx, dy, conf) field.  Start from row block F-1 of stack 0; for level = F-1 .. 1 do the step of
 * ugsm_reconstruct_full from level to level-1 with this window test: a pixel of level-1 inside window k takes stack k's value -- where
 * several windows hold it, the HIGHEST k -- and a pixel inside no window takes the upsample, all three channels scaled.  A pasted pixel never
 * computes the upsample.  n == 1: bit for bit ugsm_reconstruct_full.  fovea_levels < 2, n outside 1 .. UGSM_MAX_BATCH, null entries:
 * UGSM_ERR_BAD_ARG.  Asynchronous on `slot`. */
int ugsm_reconstruct_full_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H,
                                const int *off_x, const int *off_y, float *d_out3);

/* ---- the warped right image and the photometric residual of a match ----------------------------------------------------------------
 *
 * MatchGPULib::warpRightImage (MatchGPULib.h:40, MatchGPULib.cpp:1445-1518, stage `warp` / kernel warpAbyB, MatchLib.cu:499-549) on device
 * memory, and the number that goes with the picture: whether, without ground truth, the right image lands on the left one under a field.
 *
 * THE WARP.  For a W x H plane src and fields dx, dy of the same size
 *   warp(src, dx, dy)[iy][ix] = src[ tex(((float)iy + 0.5f) + dy[iy][ix], H) ][ tex(((float)ix + 0.5f) + dx[iy][ix], W) ]
 * with tex(f, n) the matcher's texture index: floor(f); !(floor >= 0), NaN included, gives 0; floor > n-1 gives n-1.  The sums are binary32,
 * each rounded on its own; the fetched value is stored as it is, with no arithmetic on it.  For finite and for wild disparities (NaN, +-inf,
 * +-3e38, +-2^31, denormals) this is, bit for bit, the reference's `warp` with texSrc = src, texdispx = dx, texdispy = dy, and the matcher's
 * own fetch of the right image inside an iteration.
 *
 * THE RESIDUAL.  Left planes L_c, right planes R_c (c = 0, 1, 2), fields dx, dy and weights conf (NULL: every weight is 1.0f).  With
 * R'_c = warp(R_c, dx, dy), the per-pixel term is t = fabsf(L_c - R'_c) in float, then t = t * conf in float; S_c = sum(t) per channel and
 * C = sum(conf).  The four sums are binary64, in the fixed order of weightedDifference as this build defines it (row f-4,
 * ugsm_stage_weighted_difference): within a row, lane l = x mod 64 adds its columns left to right from 0.0, and the 64 lane sums are then
 * added in lane order from 0.0; the row sums go the same way over y mod 64.  So (float)(S_a / C) is what ugsm_stage_weighted_difference
 * returns for the fields (L_a, L_b, conf) and (R'_a, R'_b, .).  No float atomics anywhere: the same bytes come out from run to run.  The
 * device writes S_0, S_1, S_2, C as four doubles; the host forms S_c / C, and C == 0 is the host's business.  A mono8 context: S_0 = S_1 = S_2.
 *
 * All five calls are asynchronous on `slot`'s stream, like ugsm_triangulate -- so ordered behind a ugsm_submit_* on the same slot -- and
 * make no host synchronisation unless a scratch buffer has to grow.  The residual's row sums (4 doubles per row and level) live in a
 * per-slot scratch that grows on demand, counted by ugsm_context_device_bytes; UGSM_ERR_NOMEM if it cannot grow, and the context stays
 * usable.  The images are read in the context's input format, captured at the call (ugsm_set_input_format).
 * UGSM_ERR_STATE while pairs enqueued with ugsm_enqueue_* are outstanding.  UGSM_ERR_BAD_ARG, before any device work: a null pointer
 * (d_conf / d_stackc excepted), W or H < 1, H above 65535, more than 2^28 pixels, stride < bytes per pixel * W, channels outside 1 .. 96, a
 * bad slot, d_dst == d_src or d_warp == d_pyrR (the warp is not in place), a d_sums that is not 8-byte aligned, the fovea forms on a
 * context with fovea_levels < 2.
 * NOT built: a per-pixel residual map; a byte-image (rgb8) output of the warp; queue / managed forms; the stacks of several windows in one
 * call (call the stack form once per window); a residual that feeds back into the confidence. */
/* planes in, planes out: MatchGPULib::warpRightImage on device memory.  channels planes of W x H floats, one (dx, dy) for all of them */
int ugsm_warp_planes(ugsm_ctx *ctx, int slot, const float *d_src, int channels, int W, int H,
                     const float *d_dispx, const float *d_dispy, float *d_dst);
/* the right IMAGE as it is on the device (the context's input format) -> three float planes R', G', B' of the warped image, 3 x H x W
 * floats; mono8: three equal planes.  No float copy of the image is made first. */
int ugsm_warp_right(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbR, int W, int H, int stride,
                    const float *d_dispx, const float *d_dispy, float *d_warp3);
/* every level of a fovea stack in ONE launch: level k of d_pyrR ((F*3*fovH) x fovW floats, rows [level][channel][row], as
 * ugsm_submit_foveated writes it) warped by level k of d_stackx / d_stacky ((F*fovH) x fovW), clamped to the fovW x fovH window as the
 * matcher's own fetch is; d_warp is laid out as d_pyrR.  F is the context's fovea_levels. */
int ugsm_warp_right_fovea(ugsm_ctx *ctx, int slot, const float *d_pyrR, const float *d_stackx, const float *d_stacky,
                          int fovW, int fovH, float *d_warp);
/* the residual of a full-resolution field, straight from the two images (no warped image is stored); d_conf may be NULL; d_sums4: 4
 * doubles on the device, 8-byte aligned: S_0, S_1, S_2, C */
int ugsm_photometric_residual(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride,
                              const float *d_dispx, const float *d_dispy, const float *d_conf, double *d_sums4);
/* the same per level of a stack, one launch for the rows of all levels and one for the totals; d_stackc may be NULL; d_sums: F x 4
 * doubles, [level][S_0, S_1, S_2, C] */
int ugsm_photometric_residual_fovea(ugsm_ctx *ctx, int slot, const float *d_pyrL, const float *d_pyrR, const float *d_stackx,
                                    const float *d_stacky, const float *d_stackc, int fovW, int fovH, double *d_sums);

/* ---- stage-level entry points (tests only; device pointers; synchronous) -------- */
/* (the probes of the kernels' exact arithmetic shortcuts -- ugsm_stage_poly_probe, ugsm_stage_div3_probe, ugsm_stage_div_probe -- are
 * declared in include/ugsm_dev.h and exported by libugsm_dev.so only) */

/* CreatePyramidFromImage, MatchGPULib.cpp:1033-1125: builds the pyramid of one rgb8
 * image in `slot`'s left pyramid and copies level `level` (3 planes) to d_out3. */
int ugsm_stage_pyramid(ugsm_ctx *ctx, const uint8_t *d_rgb, int W, int H, int stride, int level,
                       float *d_out3);
/* matchlevel, MatchGPULib.cpp:1662-2489: iterations m_from..m_to of a level with mi
 * iterations and S smoothing passes.  d_dbg8 (may be NULL): 5 Q planes + dx',dy',kappa
 * before smoothing, of the last iteration run (kernel_path 1 only). */
int ugsm_stage_iterate(ugsm_ctx *ctx, const float *d_L3, const float *d_R3, float *d_d3, int W,
                       int H, int mi, int S, int is_top, int m_from, int m_to, float *d_dbg8);
/* subsampleDisp / foveatedsubsampleDisp, MatchGPULib.cpp:1526-1655 */
int ugsm_stage_seed(ugsm_ctx *ctx, const float *d_src3, int W, int H, float *d_dst3, int W2, int H2,
                    int Wup, int Hup, int crop_x, int crop_y);
/* The restriction of the seeded call (ugsm_submit_full_seeded) alone: level `level`'s starting field d_dst3 (3 planes of w x h, the level's
 * size by ugsm_level_dims with the context's levels) from the full-resolution field d_src3 (3 planes of W x H).  Not in place. */
int ugsm_stage_restrict(ugsm_ctx *ctx, const float *d_src3, int W, int H, int level, float *d_dst3);
/* The prolongation of the coarse half (ugsm_submit_full_coarse) alone: the full-resolution field d_dst3 (3 planes of W x H) from level `level`'s
 * field d_src3 (3 planes of w x h, the level's size by ugsm_level_dims with the context's levels), one launch.  Not in place. */
int ugsm_stage_prolong(ugsm_ctx *ctx, const float *d_src3, int W, int H, int level, float *d_dst3);
/* The starting-field launch of the warm foveated call (ugsm_submit_foveated_warm) alone: row blocks start_level .. F-1 of d_dst_stack from the
 * stack d_prior_stack matched at (prior_off_x, prior_off_y), for a window at (off_x, off_y); the row blocks below are not written.  Not in place. */
int ugsm_stage_warm_stack(ugsm_ctx *ctx, const float *d_prior_stack, int W, int H, int prior_off_x, int prior_off_y, int off_x, int off_y,
                          int start_level, float *d_dst_stack);
/* S smoothing passes (+ box if do_box), MatchGPULib.cpp:2257-2412, in place */
int ugsm_stage_smooth(ugsm_ctx *ctx, float *d_d3, int W, int H, int passes, int do_box);

/* Row f-4: weightedDifference (MatchGPULib.cpp:1336-1437) of two device (dx, dy, conf) fields, weights = the new field's
 * conf: out2[0] = dx, out2[1] = dy (host).  Fixed-order binary64 sums, identical to the CPU restatement. */
int ugsm_stage_weighted_difference(ugsm_ctx *ctx, const float *d_new3, const float *d_old3, int W, int H, float *out2);
/* The LR-consistency check (ugsm_config.lr_check_threshold; no reference counterpart) on two device (dx, dy, conf) fields: zeroes
 * d_left3's confidence where d_right3 does not point back within tau; *marked (host, may be NULL) = number of pixels marked. */
int ugsm_stage_lr_check(ugsm_ctx *ctx, float *d_left3, const float *d_right3, int W, int H, float tau, long long *marked);
/* Pixels the LR check of the last full-mode call on `slot` marked (-1: the call ran without the check; a batched call, which such a
 * context runs pair by pair: of its last pair).  After a checked foveated call (UGSM_LR_FOVEATED): the sum over the levels of the call's
 * last pair.  Valid after ugsm_wait. */
long long ugsm_last_lr_marked(ugsm_ctx *ctx, int slot);
/* The same level by level, for pair `pair` of the last call on `slot`: per_level[0 .. fovea_levels).  UGSM_ERR_STATE if that call ran
 * without the foveated check, UGSM_ERR_BAD_ARG for a bad slot or pair or a null pointer.  Valid after ugsm_wait. */
int ugsm_last_lr_marked_levels(ugsm_ctx *ctx, int slot, int pair, long long *per_level);
/* Pixels the check of the last ugsm_submit_full_checked / ugsm_match_full_checked on `slot` marked for pair `pair`: *fwd in the left-to-right
 * field, *back in the right-to-left one (either may be NULL).  UGSM_ERR_STATE if the last call on the slot was another one, UGSM_ERR_BAD_ARG
 * for a null context, a bad slot or a bad pair.  Valid after ugsm_wait. */
int ugsm_last_lr_marked_pair(ugsm_ctx *ctx, int slot, int pair, long long *fwd, long long *back);
/* Iterations each level of the last call on `slot` actually ran (early_exit_threshold > 0 can stop a level early);
 * per_level[UGSM_MAX_LEVELS], -1 for levels not run.  ugsm_stage_iterate records its count at index 0. */
int ugsm_last_iterations(ugsm_ctx *ctx, int slot, int *per_level);

/* ---- instrumentation ------------------------------------------------------------ */

typedef struct ugsm_kernel_stat {
    char name[48];
    int level;              /* pyramid level the launches belong to; -1: none (stage entry points, copies) */
    int reserved;
    long long launches;
    double total_ms;        /* sum of HIP-event durations (profile_events, slot 0) */
    double pixel_launches;  /* sum over launches of pixels processed */
} ugsm_kernel_stat;

/* One entry per (kernel, pyramid level) with at least one harvested launch (launches are harvested by ugsm_wait).
 * Fills up to `cap` entries; returns the number of entries there are. */
int ugsm_get_kernel_stats(ugsm_ctx *ctx, ugsm_kernel_stat *out, int cap);
int ugsm_reset_kernel_stats(ugsm_ctx *ctx);
/* Changes ugsm_config.profile_events of a live context (0 off, 1 cost kernels, 2 every kernel); takes effect for
 * launches enqueued afterwards.  bench.py times its throughput region with events off and reads kernel durations
 * from a separate single-pair pass. */
int ugsm_set_profile_events(ugsm_ctx *ctx, int mode);

/* Device memory the context holds right now in its slots' buffers (pyramids, fields, staging; they grow on demand and are kept):
 * about 1.35 GB per pair of a call and slot at 16 MP, i.e. slots x batch x 1.35 GB once every slot has run a full-size call
 * (four slots, batch 8: 43 GB; batch 16: 86 GB of the 288).  -1 for a null context. */
long long ugsm_context_device_bytes(const ugsm_ctx *ctx);

/* Device-memory helpers so a C/C++ host (the ROS node) needs no HIP headers. */
int ugsm_dev_alloc(ugsm_ctx *ctx, void **d_ptr, long long bytes);
int ugsm_dev_free(ugsm_ctx *ctx, void *d_ptr);
/* Page-locked host memory (optional): images and result planes placed here make the host<->device copies
 * of ugsm_match_full / ugsm_match_foveated plain DMA (the reference's node mallocs and frees its planes,
 * UG_GPU_matcher.cpp:414-418; a node that adopts these two calls keeps them for the life of the context). */
int ugsm_host_alloc(ugsm_ctx *ctx, void **h_ptr, long long bytes);
int ugsm_host_free(ugsm_ctx *ctx, void *h_ptr);
int ugsm_copy_to_device(ugsm_ctx *ctx, void *d_dst, const void *h_src, long long bytes);
int ugsm_copy_to_host(ugsm_ctx *ctx, void *h_dst, const void *d_src, long long bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* UGSM_H */
