/*
 * orbfe.h — C-ABI of the MI355X-native ORB front-end (liborbfe.so, gfx950 HIP).
 *
 * Drop-in boundary for the pyOrbSLAM2 front-end hot path.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo M2219/pyOrbSLAM):
 *
 *   pyORBExtractor.ORBextractor            pyORBExtractor/orb_extractor.cpp:22-38, ORBextractor.h:45-114
 *   Frame.compute_stereo_matches           Frame.py:161-279
 *   ORBMatcher.descriptor_distance / search_by_projection_f_f / _f_p (Hamming core)
 *                                          ORBMatcher.py:12-14, 215-283, 291-393
 *   pyDBoW.TemplatedVocabulary load_from_text_file / transform / transform_feature
 *                                          pyDBoW/TemplatedVocabulary.py:43-81, 108-160
 *
 * Conventions
 *   - plain C types only; caller-owned output buffers; every call returns an int status
 *     (ORBFE_OK = 0, < 0 on error) and the message is kept in a thread-local string
 *     readable with orbfe_last_error();
 *   - one handle per camera / per thread (the reference extractor is stateful and not
 *     re-entrant: ORBextractor.h:88 overwrites mvImagePyramid on every call);
 *   - "device" entry points take device pointers and a hipStream_t passed as void*;
 *     they enqueue work and return without synchronising.
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header (orbfe_abi_version() returns the library's).  4: ORBFE_NSTAGES = 5 (stage 3
 * describe, 4 stereo; the round-1 blur stage and orbfe_set_blur_fork are gone), orbfe_set_graphs,
 * orbfe_set_octree_kernel / orbfe_get_octree_kernel, orbfe_debug_detect_stats. */
#define ORBFE_ABI_VERSION 9 /* 6: compact gather records pack x | y << 14 | octave << 28 (was 12 / 12 / 24); level
                               * sides above 4 095 px are accepted (kKeyXYBits).  7: orbfe_kfdb_*, orbfe_bow_score.
                               * 8: orbfe_vocab_bow, orbfe_vocab_bow_device, orbfe_vocab_bow_scratch_bytes,
                               * orbfe_vocab_bow_last_ms (additive).  9: orbfe_get_stereo_bucket_kernel (additive).
                               * Still 9: orbfe_bow_match, orbfe_bow_match_device, orbfe_bow_match_last_ms and
                               * orbfe_bow_match_out only add entry points and a struct; find them by symbol.
                               * Likewise orbfe_tri_match, orbfe_tri_match_last_ms and orbfe_tri_match_out, and
                               * orbfe_fuse_search, orbfe_fuse_search_last_ms and orbfe_fuse_out, and
                               * orbfe_kfdb_query_many, orbfe_kfdb_query_many_device, orbfe_kfdb_set_scratch_limit,
                               * orbfe_kfdb_many_last_ms and orbfe_kfdb_many_out, and orbfe_scw_search,
                               * orbfe_scw_search_last_ms and orbfe_scw_out, and orbfe_sim3_search,
                               * orbfe_sim3_search_last_ms and orbfe_sim3_out, and orbfe_fkf_search,
                               * orbfe_fkf_search_last_ms and orbfe_fkf_out, and orbfe_debug_detect_lanes, and
                               * orbfe_local_search, orbfe_local_search_last_ms and orbfe_local_out, and
                               * orbfe_ff_search, orbfe_ff_search_last_ms and orbfe_ff_out */
/* frames whose sheared pyramids the lazy frame path (want_pyramid = 2) keeps on the device */
#define ORBFE_FRAME_RING 8
int32_t orbfe_abi_version(void);

#define ORBFE_OK 0
#define ORBFE_EINVAL (-1)    /* bad argument / unsupported configuration            */
#define ORBFE_ENOMEM (-2)    /* host or device allocation failed                    */
#define ORBFE_EHIP (-3)      /* HIP runtime error (message from hipGetErrorString)   */
#define ORBFE_ECAPACITY (-4) /* caller buffer too small (*n_out holds the need)     */
#define ORBFE_ESTATE (-5)    /* call order violated (e.g. pyramid before extract)   */
#define ORBFE_EOVERFLOW (-6) /* an on-device capacity bound was exceeded            */
#define ORBFE_EFORMAT (-7)   /* malformed input file (vocabulary text)              */
#define ORBFE_EREJECT (-8)   /* vocabulary header outside the accepted ranges       */

/* ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (orb_extractor.cpp:23; ORBextractor.cpp:410-470). */
typedef struct orbfe_params {
    int32_t nfeatures;
    float scale_factor; /* narrowed to float exactly like the pybind11 float argument */
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    /* Lane count of OpenCV's vectorised vertical resize pass (cv::resize INTER_LINEAR 8U,
     * SURVEY.md Appendix A.2 / H2): 16 = CV_SIMD128 baseline build (default), 32 = AVX2-wide
     * build, 0 = scalar formula everywhere.  OpenCV is not vendored by the reference; this is
     * the only unpinned knob of the pixel arithmetic. */
    int32_t resize_simd_lanes;
} orbfe_params;

/* cv::KeyPoint as the reference's caster returns it: (pt.x, pt.y, size, angle, response,
 * octave) (opencv_type_casters.h:106-108).  24 bytes, naturally aligned. */
typedef struct orbfe_keypoint {
    float x, y, size, angle, response;
    int32_t octave;
} orbfe_keypoint;

typedef struct orbfe_ctx* orbfe_handle;

/* ---- lifetime ------------------------------------------------------------------------ */

/* ORBextractor::ORBextractor (ORBextractor.cpp:410-470). */
int orbfe_create(const orbfe_params* params, orbfe_handle* out);
int orbfe_destroy(orbfe_handle h);
const char* orbfe_last_error(void);
/* library build string ("gfx950 ...") */
const char* orbfe_version(void);

/* Build identity: the first 16 hex digits of the SHA-256 of the sources and headers the library was built
 * from (Makefile).  Measurement files (profiles/traffic.json, profiles/valu.json) record it, and bench.py
 * uses their per-kernel figures only when it matches the loaded library. */
const char* orbfe_build_id(void);

/* GetLevels/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/
 * GetInverseScaleSigmaSquares (ORBextractor.h:62-82).  Each array has nlevels floats; any
 * pointer may be NULL.  n_per_level receives mnFeaturesPerLevel (ORBextractor.cpp:435-446). */
int orbfe_get_scales(orbfe_handle h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                     int32_t* n_per_level);

/* ---- host-buffer drop-in (one image per call) ------------------------------------------ */

/* ORBextractor::operator_kd (ORBextractor.cpp:1042-1104) as bound at orb_extractor.cpp:31-38.
 * img: width x height u8, row stride `stride` bytes (the reference ignores numpy strides and
 * requires C-contiguous input; pass stride = width for identical behaviour).
 * Writes up to `cap` keypoints and cap*32 descriptor bytes; *n_out = number produced.
 * An empty image (width or height 0) yields *n_out = 0 (ORBextractor.cpp:1045-1046). */
int orbfe_extract(orbfe_handle h, const uint8_t* img, int32_t width, int32_t height, int32_t stride,
                  orbfe_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out);

/* GetImagePyramid (orb_extractor.cpp:30): pyramid level `level` of the last orbfe_extract.
 * sheared = 1 reproduces the reference's Mat->ndarray caster, which ignores Mat::step and so
 * returns row r of a level as bytes [19*(w+38)+19 + r*w, ... + w) of the 19-px reflect-101
 * padded buffer (opencv_type_casters.h:232-239; ORBextractor.cpp:1112-1128);
 * sheared = 0 returns the true w x h level.  out must hold w*h bytes (sizes via w_out, h_out;
 * call with out = NULL to query the size). */
int orbfe_pyramid(orbfe_handle h, int32_t level, uint8_t* out, int32_t sheared, int32_t* w_out,
                  int32_t* h_out);

/* Frame.compute_stereo_matches (Frame.py:161-279) on the last left/right extraction of two
 * handles (left = hl, right = hr; both must have extracted same-size images).
 * bf = Frame.mbf (Python float), fx = Frame.mK[0][0] (np.float32).
 * Outputs, each of length nL = number of left keypoints:
 *   status[i] = 0  no match      (reference keeps Python int -1)
 *             = 1  matched       (reference stores np.float32 uR / depth: u_right / depth)
 *             = 2  zero disparity: the reference substitutes disparity = 0.01 in Python double
 *                  precision (Frame.py:273-275); u_right/depth then hold uL-0.01 and bf/0.01
 *                  rounded to f32 and the host layer recomputes them in double.
 *   match_r[i] = index of the right keypoint chosen by the Hamming search (or -1). */
int orbfe_stereo_match(orbfe_handle hl, orbfe_handle hr, double bf, float fx, float* u_right, float* depth,
                       int8_t* status, int32_t* match_r, int32_t n_left);

/* ---- per-frame stereo path (one Frame, one enqueue) ------------------------------------------
 * Frame.__init__ (Frame.py:48-65) calls ExtractORB(0, left), ExtractORB(1, right) — two synchronous
 * operator_kd calls, ORBextractor.cpp:1042-1104 — then GetImagePyramid on both extractors
 * (orb_extractor.cpp:30) and compute_stereo_matches (Frame.py:161-279).  orbfe_frame_extract does all
 * of it for one stereo pair in ONE enqueue on the handle's stream: both images copied in, the 2-image
 * pipeline, the stereo match, optionally the sheared pyramids of both images (built on the device), and
 * every result copied into page-locked host memory before a single synchronisation.  The fetch calls
 * below then only copy host memory.  Both images are width x height u8 with row stride `stride`; an
 * empty image (width or height 0) yields no keypoints (ORBextractor.cpp:1045-1046).  bf / fx as in
 * orbfe_stereo_match.  want_pyramid: 0 none (orbfe_frame_pyramid builds them on request), 1 the sheared
 * views copied into the frame buffer with the results, 2 lazy: the views stay in a device ring of
 * ORBFE_FRAME_RING frames and cross PCIe only when orbfe_frame_pyramid_fetch asks for them (Frame.py:59-60
 * keeps the lists, but the tracking loop rarely reads them). */
int orbfe_frame_extract(orbfe_handle h, const uint8_t* left, const uint8_t* right, int32_t width, int32_t height,
                        int32_t stride, double bf, float fx, int32_t want_pyramid);
/* keypoints / descriptors of side 0 (left) or 1 (right) of the last frame (operator_kd's outputs) */
int orbfe_frame_fetch(orbfe_handle h, int32_t side, orbfe_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out);
/* stereo results of the last frame (layout and meaning as orbfe_stereo_match; *n_out = left count) */
int orbfe_frame_fetch_stereo(orbfe_handle h, float* u_right, float* depth, int8_t* status, int32_t* match_r,
                             int32_t cap, int32_t* n_out);
/* GetImagePyramid()[level] of side 0 / 1 of the last frame: the reference's sheared view (see
 * orbfe_pyramid).  Built at extraction when want_pyramid was set, otherwise now.  out = NULL queries
 * the size. */
int orbfe_frame_pyramid(orbfe_handle h, int32_t side, int32_t level, uint8_t* out, int32_t* w_out, int32_t* h_out);
/* serial number of the last frame (1, 2, ...) and the oldest serial the ring can still hold (a frame extracted
 * with want_pyramid != 2, or before a geometry change, is not in it) */
int orbfe_frame_serial(orbfe_handle h, int64_t* serial, int64_t* oldest);
/* both sheared pyramids' bytes of side 0 / 1 of frame `serial` (extracted with want_pyramid = 2): every
 * level's w_l x h_l view at its shear offset (levels concatenated, 4-byte aligned; bytes = the geometry's
 * shear size, orbfe_batch_view_get).  ORBFE_ESTATE once ORBFE_FRAME_RING newer frames have replaced it. */
int orbfe_frame_pyramid_fetch(orbfe_handle h, int64_t serial, int32_t side, uint8_t* out, int64_t bytes);

/* cv::undistortPoints(pts, K, D, noArray(), K) as Frame.undistort_keypoints (Frame.py:306) and
 * Tracking.compute_image_bounds (Tracking.py:132) call it: OpenCV 4.x's 5-iteration fixed point in double
 * (k_undistort).  K4 = (fx, fy, cx, cy) and dist = (k1, k2, p1, p2[, k3]) as float (the reference keeps
 * mK and mDistCoef in float32); xy: n points at `stride` floats apart (x, y first); out: n x 2 floats.
 * Parity is unpinned: OpenCV is absent and the reference's distorted branch is unreachable (NameError
 * on `mvKeys` at Frame.py:299); DESIGN.md §2 states the semantics followed. */
int orbfe_undistort_points(orbfe_handle h, const float* K4, const float* dist, int32_t n_dist, const float* xy, int32_t n,
                           int32_t stride, float* out);

/* ---- device batch API (bench / batched-frames mode) ----------------------------------------
 * Images are device-resident, n_images x (height x img_pitch) u8, stereo pair p = images
 * (2p, 2p+1) = (left, right).  Results stay on device in handle-owned buffers. */

/* Allocate device workspace for up to max_images images of width x height (idempotent for the
 * same geometry). */
int orbfe_batch_reserve(orbfe_handle h, int32_t width, int32_t height, int32_t max_images);

/* Run the whole extractor on n_images device images (no host synchronisation). */
int orbfe_extract_batch_device(orbfe_handle h, const uint8_t* d_images, int64_t img_pitch, int32_t n_images,
                               void* hip_stream);

/* Stereo-match n_pairs pairs of the last batch extraction (images 2p, 2p+1). */
int orbfe_stereo_batch_device(orbfe_handle h, int32_t n_pairs, double bf, float fx, void* hip_stream);

/* Convenience: extract + stereo for n_pairs pairs in one enqueue (the benchmark step). */
int orbfe_frontend_batch_device(orbfe_handle h, const uint8_t* d_images, int64_t img_pitch, int32_t n_pairs,
                                double bf, float fx, void* hip_stream);

/* orbfe_set_lanes: orbfe_frontend_batch_device runs its batch as min(lanes, n_pairs) contiguous chunks,
 * each on an internal stream (fork from / join into the caller's stream); 1..4, default 4.  Results and
 * their layout do not depend on it. */
int orbfe_set_lanes(orbfe_handle h, int32_t lanes);

/* orbfe_set_graphs(mask): which enqueues run as a HIP graph, captured on the first call with a given
 * (buffers, pointers, sizes, bf, fx) key and replayed with one hipGraphLaunch afterwards (up to 8 cached
 * graphs per handle, dropped when the handle's buffers are reallocated): ORBFE_GRAPH_FRAME =
 * orbfe_frame_extract (default: the per-frame path runs on one stream, a graph saves its launches),
 * ORBFE_GRAPH_BATCH = orbfe_frontend_batch_device with one lane (off by default: graph launches of handles on
 * different streams measured to serialise their chains, 0.27 -> 0.40 ms for 8 pairs as 4 handles).  0 =
 * every operation launched on the stream.  Results do not depend on it; profiling (orbfe_profile_begin)
 * always takes the stream path.  orbfe_graph_stats: captures and graph launches so far, graphs cached now
 * (any pointer may be NULL). */
#define ORBFE_GRAPH_FRAME 1
#define ORBFE_GRAPH_BATCH 2
int orbfe_set_graphs(orbfe_handle h, int32_t mask);
int orbfe_graph_stats(orbfe_handle h, int64_t* captures, int64_t* launches, int32_t* cached);

/* Device result layout of the last batch (pointers into handle-owned device memory):
 *   kps   : n_images x cap  orbfe_keypoint   (cap = *kp_cap)
 *   desc  : n_images x cap x 32 u8
 *   count : n_images int32
 *   u_right, depth : n_pairs x cap float; status : n_pairs x cap int8; match_r : n_pairs x cap int32 */
typedef struct orbfe_batch_view {
    int32_t kp_cap;
    int32_t n_images;
    int32_t n_pairs;
    orbfe_keypoint* kps;
    uint8_t* desc;
    int32_t* count;
    float* u_right;
    float* depth;
    int8_t* status;
    int32_t* match_r;
    int32_t* overflow; /* device int: non-zero if a capacity bound was hit in the last batch */
} orbfe_batch_view;
int orbfe_batch_view_get(orbfe_handle h, orbfe_batch_view* view);

/* Synchronise the handle's last stream and read the overflow word of the last batch (0 = every
 * on-device capacity bound held; otherwise the OR of the codes of the bounds that were hit). */
int orbfe_batch_status(orbfe_handle h, int32_t* overflow);

/* Batched-frames mode, multi-GPU: every pair's results as one fixed-capacity byte record, packed on the
 * device for the rank-0 gather (north star: "RCCL over xGMI only for the trivial gather of per-frame
 * keypoints").  Record layout (pyorbslam_amd/dist.py): counts L, R (2 x i32) | keypoints L, R
 * (kp_cap x orbfe_keypoint each) | descriptors L, R (kp_cap x 32 B each) | u_right, depth (kp_cap x f32)
 * | status (kp_cap x i8), padded to 16 bytes: orbfe_batch_record_bytes.  orbfe_batch_pack_device writes
 * pairs [pair0, pair0 + n_pairs) of the last stereo batch to d_records (n_pairs x rec_bytes, 4-byte
 * aligned) on hip_stream, without synchronising.  d_records is device memory or page-locked host memory
 * (hipHostMalloc): the records then go over PCIe straight into host memory (no device staging buffer, no
 * copy-engine transfer); pageable memory is refused with ORBFE_EINVAL.
 * Ordering (both pack calls): on the batch's own stream the pack simply follows it.  On another stream the
 * pack waits on an event recorded on the batch's stream WHEN THE PACK IS CALLED, so (a) that stream must
 * still exist and must not be inside a graph capture at that moment, and (b) whatever was queued on it after
 * the batch and before the pack call is waited for too. */
int orbfe_batch_record_bytes(orbfe_handle h, int64_t* bytes);
/* Compact records (the host-fed D2H leg and the rank-0 gather, 25 % smaller): counts L, R (2 x i32) |
 * keypoints L, R (kp_cap x {u32 x | y << 14 | octave << 28 in the keypoint's level pixels, f32 angle}) |
 * descriptors L, R (kp_cap x 32 B) | u_right, depth (kp_cap x f32) | FAST scores L, R (kp_cap x u8) | status
 * (kp_cap x i8), padded to 16 bytes (8 + 91 kp_cap).  The keypoint tuples follow exactly: x = f32(level x) *
 * scale[octave] (ORBextractor.cpp:1094-1099), size = (float)(int)(31 * scale[octave]), response = score
 * (pyorbslam_amd.dist.unpack_compact).  Device memory only. */
int orbfe_batch_compact_record_bytes(orbfe_handle h, int64_t* bytes);
int orbfe_batch_pack_compact_device(orbfe_handle h, uint8_t* d_records, int64_t rec_bytes, int32_t pair0,
                                    int32_t n_pairs, void* hip_stream);
int orbfe_batch_pack_device(orbfe_handle h, uint8_t* d_records, int64_t rec_bytes, int32_t pair0, int32_t n_pairs,
                            void* hip_stream);

/* Copy the results of image `image` (and of pair image/2 when image is even and a stereo
 * batch ran) of the last batch to host buffers.  Synchronises the handle's last stream. */
int orbfe_batch_fetch(orbfe_handle h, int32_t image, orbfe_keypoint* kps, uint8_t* desc, int32_t cap,
                      int32_t* n_out);

/* Copy the stereo results of pair `pair` of the last batch (see orbfe_stereo_match for the meaning
 * of the arrays; *n_out = left keypoint count of the pair).  Synchronises the last stream. */
int orbfe_batch_fetch_stereo(orbfe_handle h, int32_t pair, float* u_right, float* depth, int8_t* status,
                             int32_t* match_r, int32_t cap, int32_t* n_out);

/* ---- Hamming search (ORBMatcher core) -------------------------------------------------------
 * ORBMatcher.descriptor_distance (ORBMatcher.py:12-14): popcount(a ^ b) over 32 bytes, batched.
 * For query q the candidates are cand_idx[cand_off[q] .. cand_off[q+1]) (indices into
 * train_desc), scanned in order; the search keeps the FIRST strict minimum (best) and the
 * second-best distance with its candidate exactly as search_by_projection_f_p does
 * (ORBMatcher.py:252-274: `dist < best` shifts best into second; `elif dist < best2`).
 * Distances start at 256 (no candidate => best_idx = -1).  Host pointers; n_query may be 0. */
int orbfe_hamming_search(orbfe_handle h, const uint8_t* query_desc, int32_t n_query, const uint8_t* train_desc,
                         int32_t n_train, const int32_t* cand_off, const int32_t* cand_idx, int32_t* best_dist,
                         int32_t* best_idx, int32_t* second_dist, int32_t* second_idx);

/* Every candidate distance, in CSR order: out_dist[k] = popcount(query[q] ^ train[cand_idx[k]]) for
 * k in [cand_off[q], cand_off[q+1]).  Used by the ORBMatcher drop-in, whose control flow (already
 * matched points, stereo gate, best/second bookkeeping) depends on matches made earlier in the
 * same search and therefore stays sequential on the host. */
int orbfe_hamming_csr(orbfe_handle h, const uint8_t* query_desc, int32_t n_query, const uint8_t* train_desc,
                      int32_t n_train, const int32_t* cand_off, const int32_t* cand_idx, int32_t* out_dist);

/* ORBMatcher.descriptor_distance for ONE pair (ORBMatcher.py:12-14; Frame.py:324-326; MapPoint.py:76-78):
 * popcount(a ^ b) over 32 bytes, computed on the host (a device round trip costs more than the
 * reference's ~10 us Python call; batches go through the kernels above / below). */
int orbfe_descriptor_distance(const uint8_t* a, const uint8_t* b, int32_t* out);

/* Frame.get_features_in_area (Frame.py:373-416) for n_q queries at once, on the host: the frame's 64 x 48
 * grid (Frame.assign_features_to_grid, Frame.py:152-159) as CSR (cell (ix, iy) = cell_off[ix * rows + iy]
 * .. cell_off[ix * rows + iy + 1) into cell_idx, the reference's list order), the keypoints' pt (double
 * values of the Python floats) and octave, frame4 = (mnMinX, mnMinY, mfGridElementWidthInv,
 * mfGridElementHeightInv); query q = (x, y, r, min_level, max_level) in double.  Candidates of query q:
 * out_idx[out_off[q] .. out_off[q + 1]), in the reference's order.  ORBFE_ECAPACITY if more than cap
 * (out_off[n_q] then holds the total).  The ORBMatcher drop-in uses it when every operand is a double. */
int orbfe_grid_query(const int32_t* cell_off, const int32_t* cell_idx, int32_t cols, int32_t rows, const double* kp_x,
                     const double* kp_y, const int32_t* kp_oct, int32_t n_kp, const double* frame4, int32_t n_q,
                     const double* qx, const double* qy, const double* qr, const int32_t* qmin, const int32_t* qmax,
                     int32_t* out_off, int32_t* out_idx, int64_t cap);

/* The sequential candidate selection of the tracking searches over precomputed distances (host code), for
 * the ORBMatcher drop-in's double-typed fast path.  Queries are taken in order; query q's candidates are
 * idx[off[q] .. off[q + 1]) with Hamming distances dist[...] (orbfe_hamming_csr); u_right = the frame's
 * mvuRight as doubles (-1 for none); blocked[i] = 1 when frame slot i holds a map point with observations,
 * updated in place with q_obs[q] when query q's map point takes slot best_idx[q] (-1: no match).
 * orbfe_select_f_f: search_by_projection_f_f's inner loop and TH_HIGH test (ORBMatcher.py:348-372): stereo
 * gate |(u - mbf * invzc) - uR| > radius in double.  orbfe_select_f_p: search_by_projection_f_p's
 * (ORBMatcher.py:246-281): gate |xr - uR| > r_scaled, best / second best with their keypoint octaves and
 * the ratio test best > nnratio * second when both are on one octave. */
int orbfe_select_f_f(int32_t n_q, const int32_t* off, const int32_t* idx, const int32_t* dist, const double* u,
                     const double* invzc, const double* radius, const uint8_t* q_obs, const double* u_right,
                     uint8_t* blocked, int32_t n_frame, double mbf, int32_t th_high, int32_t* best_idx);
int orbfe_select_f_p(int32_t n_q, const int32_t* off, const int32_t* idx, const int32_t* dist, const double* xr,
                     const double* r_scaled, const int32_t* kp_octave, const uint8_t* q_obs, const double* u_right,
                     uint8_t* blocked, int32_t n_frame, double nnratio, int32_t th_high, int32_t* best_idx);

/* All-pairs Hamming distance matrix (n_a x n_b int32) — descriptor_distance batched. */
int orbfe_hamming_matrix(orbfe_handle h, const uint8_t* a_desc, int32_t n_a, const uint8_t* b_desc, int32_t n_b,
                         int32_t* out);

/* ---- image ingest (stereo_kitti.py:42-43: cv2.imread(path, cv2.IMREAD_GRAYSCALE)) ------------------
 * PNG (8-bit grey / RGB / grey+alpha / RGBA, non-interlaced) to 8-bit grey, decoded natively (zlib inflate
 * + row unfiltering; colour converted with libpng's rgb_to_gray fixed-point weights as OpenCV requests).
 * orbfe_png_decode: one image from memory; out = NULL returns the size only; `stride` bytes per out row.
 * orbfe_png_read_batch: n files of one size decoded by `threads` host threads into out (n x h x w,
 * contiguous), e.g. pinned staging for one host-to-device copy of a batch of stereo pairs. */
int orbfe_png_decode(const uint8_t* data, int64_t size, uint8_t* out, int64_t stride, int32_t* width, int32_t* height);
int orbfe_png_read_batch(const char* const* paths, int32_t n, int32_t width, int32_t height, uint8_t* out,
                         int32_t threads);

/* ---- live stage timing --------------------------------------------------------------------------
 * While profiling is on, every batch enqueued on the handle records HIP events around its stages:
 * 0 resize (all pyramid levels), 1 detect (FAST cells), 2 octree, 3 describe (k_orb: IC angle +
 * per-keypoint 7x7 blur + steered BRIEF), 4 stereo (row buckets + k_stereo).
 * orbfe_profile_read synchronises and returns the summed milliseconds per stage (ms_per_stage holds
 * ORBFE_NSTAGES floats) over the recorded batches. */
#define ORBFE_NSTAGES 5
int orbfe_profile_begin(orbfe_handle h, int32_t max_batches);
int orbfe_profile_read(orbfe_handle h, float* ms_per_stage, int32_t* n_batches);

/* Kernel micro-benchmark on the inputs of the last batch (development aid, not part of the drop-in):
 * runs stage `stage` in launch shape `variant` once to warm up and then `reps` times on the handle's last
 * stream, and returns the average ms.  Variant 0 is the launcher's automatic choice; the others force one of
 * the choices a launcher otherwise makes from the batch size.  Every accepted variant runs a production kernel
 * and leaves the stage's correct outputs behind, so the handle's results stay valid.  Any other stage or
 * variant number returns ORBFE_EINVAL.
 *
 *   stage       variant
 *   0 resize    0 / 7  one launch per level (also for batches that run the cascade)
 *               5      one launch per level, without the remainder wave
 *               6      the one-launch cascade with the automatic strip count (small batches only)
 *               100+S  the one-launch cascade with S strips, 1 <= S <= rows of the top level (or the next
 *                      count that fits the LDS)
 *   1 detect    0 automatic, 4 / 5: four cells / one cell per wave
 *   2 octree    0 automatic, 1 / 2: 256 / 512 threads per workgroup; with the per-candidate kernel
 *               selected (orbfe_set_octree_kernel): 0 only
 *   3 describe  0 automatic, 1 / 9 / 2: eight / four / two keypoints per wave (12 = 2)
 *   4 stereo    0 */
int orbfe_microbench(orbfe_handle h, int32_t stage, int32_t variant, int32_t reps, float* ms);

/* ---- diagnostics (stage outputs of the last orbfe_extract, image 0) ------------------------------
 * orbfe_debug_candidates: the level's FAST cell output in vToDistributeKeys order
 *   (ORBextractor.cpp:808-824), as (x_rel, y_rel, score) triples relative to (minBorderX, minBorderY).
 * orbfe_debug_selected: DistributeOctTree's result for the level in list order
 *   (ORBextractor.cpp:833-834), as (x_rel, y_rel, score) triples. */
int orbfe_debug_candidates(orbfe_handle h, int32_t level, int32_t* xyr, int32_t cap, int32_t* n_out);
int orbfe_debug_selected(orbfe_handle h, int32_t level, int32_t* xyr, int32_t cap, int32_t* n_out);
/* orbfe_debug_octree_profile: re-runs the last batch's octree stage with wall-clock marks (100 MHz ticks,
 * 64 per (image, level), 0 = not reached) written by each workgroup's first thread; development aid. */
int orbfe_debug_octree_profile(orbfe_handle h, int64_t* marks, int64_t n);
/* orbfe_debug_cascade_profile: re-runs the last batch's one-launch pyramid (k_resize_cascade; batches below 32
 * images) with wall-clock marks, 32 per (image, strip) (0 start, 1 level-0 rows staged, 2 + l level l begins,
 * 12 + l level l done); *n_strips = the strip count; development aid. */
int orbfe_debug_cascade_profile(orbfe_handle h, int64_t* marks, int64_t n_marks, int32_t* n_strips);
/* orbfe_debug_detect_stats: re-runs the last batch's FAST cell stage (idempotent) with counters:
 * stats[0] = cells processed, stats[1] = cells whose iniTh / minTh queues met so that the cell took the
 * one-pass path (both thresholds over the minTh queue), stats[2] = cells that fell back to minTh
 * (ORBextractor.cpp:811-815) on the two-queue path.  Development aid; results are unchanged. */
int orbfe_debug_detect_stats(orbfe_handle h, int64_t* stats);
/* orbfe_debug_detect_lanes: the same re-run in both launch shapes (four cells per wave, then one; ORBFE_ESTATE
 * should their counters differ), the first n (1 .. 7) words of: the three of orbfe_debug_detect_stats, then, on the
 * two-queue path, stats[3] = cells whose last iniTh M step carried minTh-queue entries in its idle lanes,
 * stats[4] = entries carried so, stats[5] = M steps the minTh fallbacks ran (ceil((|B| - carried) / 64) per fallback
 * cell); and for every cell with minTh < iniTh stats[6] = pre-test halves whose iniTh-queue emission was skipped
 * for having no iniTh pair.  Development aid; results are unchanged. */
int orbfe_debug_detect_lanes(orbfe_handle h, int64_t* stats, int32_t n);

/* DistributeOctTree implementation (ORBextractor.cpp:539-762; results are identical): 0 = automatic
 * (k_octree_bins, or the per-candidate k_octree when the bins' LDS carve would exceed 150 KiB), 1 = always
 * the per-candidate k_octree.  orbfe_get_octree_kernel reports the reserved geometry's choice (0 bins,
 * 1 per-candidate) and the bins kernel's LDS need. */
int orbfe_set_octree_kernel(orbfe_handle h, int32_t kernel);
int orbfe_get_octree_kernel(orbfe_handle h, int32_t* kernel, int64_t* bins_lds_bytes);

/* Where the stereo row buckets (Frame.py:170-179) of the reserved geometry are built.  Host-only, no device
 * call.  *fused = 1: orbfe_frame_extract and orbfe_frontend_batch_device build them inside the describe launch
 * (256-thread workgroups; the H + 1 row counters fit its LDS), 0: those calls launch the separate bucket kernel
 * too.  *threads (optional): the workgroup size of that separate kernel for a batch of n_images images (1 024
 * below 32 images, else 256), which orbfe_stereo_match (n_images = 2) and orbfe_stereo_batch_device always
 * launch.  Results do not depend on either. */
int orbfe_get_stereo_bucket_kernel(orbfe_handle h, int32_t n_images, int32_t* fused, int32_t* threads);

/* ---- bag-of-words vocabulary (pyDBoW/TemplatedVocabulary.py) ---------------------------
 *
 * A vocabulary tree of ORB descriptors.  Node 0 is the root; every other node has a parent with a
 * smaller id, and a node's children are ordered by id (the order TemplatedVocabulary.py:62-79 appends
 * them).  A node is a leaf when it has no children (Node.is_leaf, TemplatedVocabulary.py:19-20);
 * word ids number the nodes FLAGGED as leaves in id order (other nodes report word 0).  Parsing and
 * the node tables live on the host; the device copy is made on the first transform. */
typedef struct orbfe_vocab* orbfe_vocab_handle;

typedef struct orbfe_vocab_info {
    int32_t k, L;              /* header branching factor and depth (TemplatedVocabulary.py:46-47) */
    int32_t scoring, weighting; /* header codes n1, n2 (TemplatedVocabulary.py:48-49, 55-56)     */
    int64_t n_nodes;           /* including the root                                            */
    int64_t n_words;           /* flagged leaves: TemplatedVocabulary.size()                    */
    int32_t depth;             /* longest root-to-leaf path                                     */
    int32_t max_children;
} orbfe_vocab_info;

/* TemplatedVocabulary.load_from_text_file (TemplatedVocabulary.py:43-81), parsed natively.
 * Header "k L n1 n2"; ORBFE_EREJECT when 0<=k<=20, 1<=L<=10, 0<=n1<=5, 0<=n2<=3 fails (the
 * reference prints a message and returns False).  Each following line: parent is_leaf d0..d31
 * weight, with byte values in [0,255] and parent < node id; anything else is ORBFE_EFORMAT. */
int orbfe_vocab_load_text(const char* path, orbfe_vocab_handle* out);
/* The same tree from arrays: n_nodes entries each (entry 0 = root, its parent/desc ignored). */
int orbfe_vocab_create(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int64_t n_nodes,
                       const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc32, const double* weight,
                       orbfe_vocab_handle* out);
int orbfe_vocab_destroy(orbfe_vocab_handle v);
int orbfe_vocab_get_info(orbfe_vocab_handle v, orbfe_vocab_info* info);
/* Host copies of the node tables (any pointer may be NULL); n_nodes entries each. */
int orbfe_vocab_get_nodes(orbfe_vocab_handle v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc32, double* weight,
                          int32_t* word_id);

/* Descent of n descriptors (TemplatedVocabulary.transform_feature, TemplatedVocabulary.py:131-160):
 * from the root, move to the child at the smallest Hamming distance (first child on ties) until a
 * node without children.  word_id / weight are that node's; node_id is the node entered at depth
 * nid_level, or -1 when the descent stopped above it (the reference then keeps the previous
 * feature's value, which the caller threads; TemplatedVocabulary.py:118-123).  Host buffers,
 * synchronous. */
int orbfe_vocab_transform(orbfe_vocab_handle v, const uint8_t* desc32, int64_t n, int32_t nid_level,
                          int32_t* word_id, int32_t* node_id, double* weight);
/* Same on device pointers, enqueued on hip_stream (void* = hipStream_t) without synchronising. */
int orbfe_vocab_transform_device(orbfe_vocab_handle v, const uint8_t* d_desc32, int64_t n, int32_t nid_level,
                                 int32_t* d_word_id, int32_t* d_node_id, double* d_weight, void* hip_stream);
/* Kernel time of the last orbfe_vocab_transform (ms, HIP events), for measurement. */
int orbfe_vocab_last_ms(orbfe_vocab_handle v, float* ms);

/* BowVector and FeatureVector of whole frames, assembled on the device (TemplatedVocabulary.transform,
 * TemplatedVocabulary.py:108-129; BowVector.py:8-28; FeatureVector.py:8-19): k_vocab_descend, then k_bow_assemble
 * with one workgroup per frame, on one stream.  Per frame, with features i = 0 .. n - 1 in order:
 *   - nid_i is the node feature i's descent entered at depth nid_level, else nid_(i-1), with nid_(-1) = 0;
 *     the threading runs over every feature of the frame and restarts with every frame;
 *   - feature i is kept iff its weight > 0 (zero, negative and NaN weights drop it from both vectors);
 *   - BoW vector: the distinct word ids of the kept features, ascending; a word's raw weight is the sum of its
 *     kept features' weights in ascending feature index, sequentially, in IEEE double; total is the sum of the
 *     raw weights in ascending word id, sequentially, in IEEE double; when total > 0 every weight is raw / total;
 *   - feature vector: the distinct nid of the kept features, ascending, each with its kept feature indices
 *     ascending, as CSR: node r's indices are fv_idx[fv_end[r - 1] .. fv_end[r]) (fv_end[-1] = 0).
 * ORBFE_BOW_MAX_FRAME is the longest frame the kernel takes (its keys stay in LDS). */
#define ORBFE_BOW_MAX_FRAME 8192
/* Caller-owned output arrays: one entry per frame in n_words / n_nodes / n_kept, and per frame a block of
 * entries in the others (where the block starts and how long it is: see the two entry points).  Entries past a
 * frame's n_words (bow_*), n_nodes (fv_node, fv_end) and n_kept (fv_idx) are unspecified. */
typedef struct orbfe_bow_out {
    int32_t* n_words;   /* distinct words of the frame                                  */
    int32_t* bow_word;  /* word ids, ascending                                          */
    double* bow_weight; /* their normalised weights                                     */
    int32_t* n_nodes;   /* distinct nodes of the frame                                  */
    int32_t* fv_node;   /* node ids, ascending                                          */
    int32_t* fv_end;    /* exclusive end of each node's run in fv_idx                   */
    int32_t* fv_idx;    /* kept feature indices grouped by node, ascending in a run     */
    int32_t* n_kept;    /* kept features of the frame = entries of fv_idx               */
    int32_t* status;    /* ONE word: the OR of the ORBFE_BOW_* flags below over all frames (the caller zeroes
                         * it); may be NULL for orbfe_vocab_bow, which clamps nothing     */
} orbfe_bow_out;
#define ORBFE_BOW_OVER_OUT 1   /* a count above out_stride was clamped to it            */
#define ORBFE_BOW_OVER_MAX 2   /* a count above ORBFE_BOW_MAX_FRAME was clamped to it   */
#define ORBFE_BOW_OVER_FRAME 4 /* a count above frame_stride was clamped to it          */
#define ORBFE_BOW_NEGATIVE 8   /* a negative count was taken as 0                       */
/* Device pointers, enqueued on hip_stream (void* = hipStream_t) without synchronising and without allocating.
 * Frame f < n_frames is the d_count[f * count_stride] descriptors that start at descriptor f * frame_stride of
 * d_desc32 (16-byte aligned, as for orbfe_vocab_transform_device; ORBFE_EINVAL before any launch otherwise); the
 * counts are read on the device.  Frame f's outputs start at entry f * out_stride of the per-entry arrays of
 * *d_out (a host struct of device pointers).  A count that is negative or above out_stride, ORBFE_BOW_MAX_FRAME
 * or frame_stride is clamped and flagged in *d_out->status; nothing is read or written past the clamped length.
 * d_scratch: 8-byte aligned device memory of at least orbfe_vocab_bow_scratch_bytes bytes, free for reuse once
 * the work on hip_stream is done.  n_frames = 0 launches nothing.  With frame_stride = 2 * kp_cap and
 * count_stride = 2 on an orbfe_batch_view's desc / count this takes a stereo batch's left images. */
int orbfe_vocab_bow_device(orbfe_vocab_handle v, const uint8_t* d_desc32, int64_t frame_stride,
                           const int32_t* d_count, int64_t count_stride, int32_t n_frames, int32_t nid_level,
                           int64_t out_stride, const orbfe_bow_out* d_out, void* d_scratch, int64_t scratch_bytes,
                           void* hip_stream);
int orbfe_vocab_bow_scratch_bytes(int32_t n_frames, int64_t frame_stride, int64_t* bytes);
/* The same over host buffers, synchronous: frame f is descriptors [off[f], off[f + 1]) of desc32 (off[0] = 0,
 * non-decreasing) and its outputs are packed at entry off[f] of the per-entry arrays (off[n_frames] entries each).
 * ORBFE_EINVAL when a frame is longer than ORBFE_BOW_MAX_FRAME.  The vocabulary's own buffers, stream and events,
 * serialised among threads like orbfe_vocab_transform. */
int orbfe_vocab_bow(orbfe_vocab_handle v, const uint8_t* desc32, const int64_t* off, int32_t n_frames,
                    int32_t nid_level, const orbfe_bow_out* out);
/* Kernel time of the last orbfe_vocab_bow (descent + assembly, ms, HIP events), for measurement. */
int orbfe_vocab_bow_last_ms(orbfe_vocab_handle v, float* ms);

/* ---- training a vocabulary on the device (DBoW2's create: HKmeansStep / initiateClustersKMpp / setNodeWeights) ----
 *
 * The tree is built level by level, integer only, so the result is defined bit for bit (INTEGRATION.md has the
 * full definition; tests/vocab_train_definition.py restates it in NumPy):
 *   - D is the concatenation of the images' descriptors in image order.  Node 0 (the root) holds every index of D;
 *     nodes are numbered breadth-first (depth by depth, parents ascending, a parent's children in cluster order),
 *     NOT in DBoW2's recursion order.  A node's members stay in ascending index of D.
 *   - A node is split iff its depth < L and it has more than one member (the root iff it has any).  With n <= k
 *     members every member is a cluster of its own.  Otherwise: integer kmeans++ seeding drawn from splitmix64 of
 *     seed + (32 node + j + 1) * 0x9E3779B97F4A7C15, then Lloyd iterations (assignment to the centre at the
 *     smallest Hamming distance, lowest cluster index on ties; a centre becomes its members' bitwise majority, an
 *     exact half setting the bit as FORB.meanValue does; an emptied cluster keeps its centre) until an assignment
 *     repeats or max_iter iterations ran.  Clusters that end without members give no child.
 *   - A node without children is a leaf; word ids number the leaves in id order.
 *   - Weights: every descriptor of D descends the finished tree; Ni[w] counts the images that reach word w.
 *     TF_IDF and IDF: log(n_frames / Ni) in double on the host (0 where Ni = 0); TF and BINARY: 1.  Inner nodes 0. */
#define ORBFE_VOCAB_TRAIN_MAX_L 10
typedef struct orbfe_vocab_train_params {
    int32_t k;         /* 2 .. 20                                                       */
    int32_t L;         /* 1 .. 10                                                       */
    int32_t weighting; /* 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY                               */
    int32_t scoring;   /* 0 .. 5: stored in the header only                             */
    int32_t max_iter;  /* >= 1; 1 leaves the kmeans++ seeds as centres                  */
    int32_t reserved;  /* 0                                                             */
    uint64_t seed;
} orbfe_vocab_train_params;
/* Entry d of the per-depth arrays describes the nodes of depth d that were split. */
typedef struct orbfe_vocab_train_stats {
    int64_t n_desc, n_nodes, n_words;
    int64_t nodes_split[ORBFE_VOCAB_TRAIN_MAX_L];
    int64_t iter_sum[ORBFE_VOCAB_TRAIN_MAX_L];    /* Lloyd iterations, summed over the nodes with n > k */
    int64_t iter_max[ORBFE_VOCAB_TRAIN_MAX_L];
    int64_t capped[ORBFE_VOCAB_TRAIN_MAX_L];      /* nodes still changing at iteration max_iter         */
    int64_t empty_dropped[ORBFE_VOCAB_TRAIN_MAX_L]; /* seeded clusters that ended without members       */
    int64_t short_seeded[ORBFE_VOCAB_TRAIN_MAX_L];  /* nodes whose seeding stopped below k centres (S = 0) */
    double depth_ms[ORBFE_VOCAB_TRAIN_MAX_L];     /* stream time of the depth (HIP events), its read-backs included */
    double weight_ms;                             /* descent of D and the per-image word marks          */
    double kernel_ms;                             /* the sum of the above                               */
} orbfe_vocab_train_stats;
/* Image f < n_frames is descriptors start[f] .. start[f] + count[f] of desc32 (32 bytes each; start and count are
 * host arrays, so strided layouts with gaps are expressible); desc_on_device != 0 says desc32 is device memory.
 * Synchronous, on a stream and buffers of its own.  *out is an ordinary vocabulary handle.  stats may be NULL.
 * ORBFE_EINVAL before any device call: a parameter out of range, n_frames < 1, a negative start or count, more
 * than 2^31 - 1 descriptors in total, a null pointer (desc32 may be NULL only when every count is 0). */
int orbfe_vocab_train(const uint8_t* desc32, int32_t desc_on_device, const int64_t* start, const int32_t* count,
                      int32_t n_frames, const orbfe_vocab_train_params* params, orbfe_vocab_handle* out,
                      orbfe_vocab_train_stats* stats);
/* Writes the text layout orbfe_vocab_load_text reads: "k L scoring weighting", then per node after the root
 * "parent is_leaf d0 .. d31 weight", the weight as the shortest decimal that round-trips the double.  Host only. */
int orbfe_vocab_save_text(orbfe_vocab_handle v, const char* path);

/* ---- BoW-guided matching of many frame pairs (ORBMatcher.search_by_BoW_kf_f / _kf_kf, ORBMatcher.py:21-213) ----
 *
 * k_bow_match, one launch for n_pairs pairs (frame 1, frame 2) of one set of frames.  A frame is n descriptors, n
 * float angles, optionally one eligibility byte per feature and side (non-zero = eligible, a NULL array = all),
 * and a feature vector in orbfe_bow_out's CSR layout: nodes strictly ascending, every feature index in at most one
 * run.  A frame may be in many pairs, on either side, and paired with itself.  Per pair and per node both frames
 * hold, frame 1's run is walked in order; an eligible i1 looks at the i2 of frame 2's run, in run order, that are
 * eligible and not yet matched in this pair: best1 = the smallest Hamming distance, best_i2 the first i2 attaining
 * it, best2 = the second smallest distance of the multiset (256 / -1 / 256 without candidates).  i1 is matched to
 * best_i2 iff best1 < th (<= th when inclusive != 0) and (double)best1 < nnratio * (double)best2 (one IEEE double
 * product).  Then best_i2 is blocked for the later i1 of the pair, and the rotation bin is
 * rint(rot * (1.0 / 30)) with rot = (double)angle1[i1] - (double)angle2[best_i2], + 360.0 when negative, bin 30
 * taken as 0 (angles outside [0, 360] can give other values: those are recorded as bin 31).
 * search_by_BoW_kf_kf is th = 50 exclusive with both sides' eligibility, _kf_f th = 50 inclusive with side 1's.
 * Keeping the three fullest bins (ORBMatcher.compute_three_maxima) is left to the caller: the reference ranks
 * equal counts with NumPy's unstable argsort.
 * The longest frame taken is ORBFE_BOW_MAX_FRAME features (the blocked flags stay in LDS).
 * Outputs per pair p, each written in full by the kernel (no pre-fill needed; entries past n untouched):
 *   match12[p * out_stride + i1] = i2 or -1 (i1 < n1)      match21[p * out_stride + i2] = i1 or -1 (i2 < n2)
 *   bin12[p * out_stride + i1]   = rotation bin or -1       hist[p * 32 + b] = matches in bin b
 *   n_raw[p] = matches of the pair */
typedef struct orbfe_bow_match_out {
    int32_t* match12;
    int32_t* match21;
    int8_t* bin12;
    int32_t* hist;
    int32_t* n_raw;
    int32_t* status; /* ONE word: the OR of the ORBFE_BOW_* flags over all pairs (the device entry's caller zeroes
                      * it; the host entry zeroes it itself and accepts NULL) */
} orbfe_bow_match_out;
#define ORBFE_BOW_BAD_PAIR 16 /* a pair named a frame outside [0, n_frames): left all-unmatched */
/* Device pointers, enqueued on hip_stream without synchronising and without allocating.  Frames are addressed as in
 * orbfe_vocab_bow_device: frame f is d_count[f * count_stride] descriptors from descriptor f * frame_stride of
 * d_desc32 (16-byte aligned), its feature vector n_nodes[f] entries from entry f * fv_stride of d_fv's fv_node /
 * fv_end / fv_idx (what orbfe_vocab_bow_device wrote with out_stride = fv_stride).  The angle of feature i of frame
 * f is d_angle[(f * frame_stride + i) * angle_stride]: angle_stride = 6 on &kps->angle of an orbfe_batch_view, 1
 * on a plain array.  Side s's eligibility of feature i of frame f is d_elig<s>[f * elig<s>_stride + i] (any
 * non-zero byte; an int8 stereo status array qualifies), NULL = all eligible.  d_pairs: n_pairs x 2 frame indices.
 * Counts are read on the device, clamped to out_stride, ORBFE_BOW_MAX_FRAME and frame_stride and flagged like
 * orbfe_vocab_bow_device's; node counts, run ends and feature indices outside a frame's clamped range are ignored,
 * so nothing is read or written past it.  A pair naming a frame outside [0, n_frames) sets ORBFE_BOW_BAD_PAIR and
 * stays unmatched.  n_pairs = 0 launches nothing. */
int orbfe_bow_match_device(const uint8_t* d_desc32, int64_t frame_stride, const int32_t* d_count, int64_t count_stride,
                           int32_t n_frames, const float* d_angle, int64_t angle_stride, const uint8_t* d_elig1,
                           int64_t elig1_stride, const uint8_t* d_elig2, int64_t elig2_stride,
                           const orbfe_bow_out* d_fv, int64_t fv_stride, const int32_t* d_pairs, int32_t n_pairs,
                           int32_t th, int32_t inclusive, double nnratio, const orbfe_bow_match_out* d_out,
                           int64_t out_stride, void* hip_stream);
/* The same over host buffers, synchronous.  Frame f is features [off[f], off[f + 1]) of desc32 / angle / elig1 /
 * elig2 (off[0] = 0); its nodes are entries [fv_off[f], fv_off[f + 1]) of fv_node / fv_end (fv_off[0] = 0, run ends
 * relative to the frame), its feature indices start at fv_idx[off[f]].  Outputs as above with out_stride >= the
 * longest frame of the pairs.  Everything is validated before any device call: ORBFE_EINVAL when nodes are not
 * strictly ascending, run ends decrease or pass the frame's length, a feature index is out of range or appears
 * twice in a frame, a pair names a frame that does not exist, a frame is longer than ORBFE_BOW_MAX_FRAME, or a
 * needed pointer is NULL.  Process-wide buffers, stream and events: concurrent callers take turns. */
int orbfe_bow_match(const uint8_t* desc32, const float* angle, const uint8_t* elig1, const uint8_t* elig2,
                    const int64_t* off, int32_t n_frames, const int64_t* fv_off, const int32_t* fv_node,
                    const int32_t* fv_end, const int32_t* fv_idx, const int32_t* pairs, int32_t n_pairs, int32_t th,
                    int32_t inclusive, double nnratio, const orbfe_bow_match_out* out, int64_t out_stride);
/* Kernel time of the last orbfe_bow_match (ms, HIP events), for measurement. */
int orbfe_bow_match_last_ms(float* ms);

/* ---- matching many keyframe pairs for triangulation (ORBMatcher.search_for_triangulation, ORBMatcher.py:584-711) ----
 *
 * k_tri_match, one launch for n_pairs pairs (frame 1, frame 2) of one set of frames.  A frame is n descriptors, n
 * float angles, n undistorted keypoint positions (x, y as doubles), n octaves, n flag bytes (below), a feature
 * vector in orbfe_bow_match's CSR layout and two thresholds per pyramid level: thr_epi[l] (3.84 * mvLevelSigma2[l]
 * in the reference) and thr_ex[l] (100 * mvScaleFactors[l]).  A pair adds F12 (9 doubles, row-major) and the
 * epipole of frame 1's camera in frame 2 (ex, ey).
 * The walk over the two feature vectors is the reference's own, done on the host inside the entry: every round
 * draws one node from BOTH vectors; equal nodes are visited, otherwise one further node of the side with the
 * smaller id is discarded.  (A node both frames hold can therefore go unvisited.)  Where that discard finds its
 * vector exhausted the reference lets StopIteration escape: the pair gets stopped[p] = 1, no work, and its
 * match12 row stays -1.
 * Inside a visited node pair frame 1's run is walked in order.  A feature takes part iff its ORBFE_TRI_ELIGIBLE bit
 * is set and, when only_stereo != 0, its ORBFE_TRI_STEREO bit too.  For i1, a candidate i2 of frame 2's run counts
 * iff it takes part, is not yet matched in this pair, its Hamming distance d <= th, and, all in IEEE double in this
 * operation order without contraction,
 *   if neither feature has ORBFE_TRI_STEREO: (ex - x2) * (ex - x2) + (ey - y2) * (ey - y2) >= thr_ex[octave2];
 *   a = x1 * F00 + y1 * F10 + F20, b = x1 * F01 + y1 * F11 + F21, c = x1 * F02 + y1 * F12 + F22,
 *   num = a * x2 + b * y2 + c, den = a * a + b * b, den != 0 and num * num / den < thr_epi[octave2].
 * i1 is matched to the counting candidate of the smallest d, on equal d the LAST in run order; there is no
 * second-best ratio.  The winner is then blocked for the later i1 of the pair and the rotation bin is computed as
 * for orbfe_bow_match.  Keeping the three fullest bins is left to the caller.
 * The reference squares with `** 2` (libm pow), which may differ from a product by one ulp.  A pair in which any
 * evaluated gate has |lhs - thr| <= thr * 2^-48 (the epipole gate is evaluated for every candidate that takes
 * part, is unmatched and has d <= th when both features are mono; the line test for those that pass it), in which
 * den is nonzero but below the smallest normal double, or in which a rotation bin falls outside [0, 30] gets
 * ORBFE_TRI_MARGINAL in status[p]: its outputs are then this arithmetic's, and the caller that wants the
 * reference's decision redoes the pair with the reference's own expressions.
 * The longest frame taken is ORBFE_BOW_MAX_FRAME features.  Outputs per pair p (entries past n1 untouched):
 *   match12[p * out_stride + i1] = i2 or -1    bin12[p * out_stride + i1] = rotation bin or -1
 *   hist[p * 32 + b] = matches in bin b        n_raw[p] = matches      status[p], stopped[p]: one word per pair */
#define ORBFE_TRI_ELIGIBLE 1 /* flag bit: the feature holds no map point            */
#define ORBFE_TRI_STEREO 2   /* flag bit: the feature has a right coordinate (mvuRight >= 0) */
#define ORBFE_TRI_MARGINAL 1 /* status bit: a decision of the pair lies within rounding of its threshold */
typedef struct orbfe_tri_match_out {
    int32_t* match12;
    int8_t* bin12;
    int32_t* hist;
    int32_t* n_raw;
    int32_t* status;  /* n_pairs words */
    int32_t* stopped; /* n_pairs words */
} orbfe_tri_match_out;
/* Host buffers, synchronous.  Frame f is features [off[f], off[f + 1]) of desc32 / angle / xy (2 doubles each) /
 * octave / flags; its nodes are entries [fv_off[f], fv_off[f + 1]) of fv_node / fv_end, its feature indices start at
 * fv_idx[off[f]], its levels are entries [lvl_off[f], lvl_off[f + 1]) of thr_epi / thr_ex (all three offset arrays
 * start at 0).  pairs: n_pairs x 2 frame indices; F12: n_pairs x 9; epipole: n_pairs x 2.  out_stride >= the longest
 * frame 1 of the pairs.  Everything is validated before any device call, as for orbfe_bow_match, and also:
 * ORBFE_EINVAL when an octave lies outside its frame's level table, or a coordinate, threshold, F12 or epipole is
 * not finite (the message names the frame or pair), or th is outside [0, 256].  Process-wide buffers, stream and
 * events of its own: concurrent callers take turns. */
int orbfe_tri_match(const uint8_t* desc32, const float* angle, const double* xy, const int32_t* octave,
                    const uint8_t* flags, const int64_t* off, int32_t n_frames, const int64_t* fv_off,
                    const int32_t* fv_node, const int32_t* fv_end, const int32_t* fv_idx, const int64_t* lvl_off,
                    const double* thr_epi, const double* thr_ex, const int32_t* pairs, const double* F12,
                    const double* epipole, int32_t n_pairs, int32_t th, int32_t only_stereo,
                    const orbfe_tri_match_out* out, int64_t out_stride);
/* Kernel time of the last orbfe_tri_match (ms, HIP events), for measurement. */
int orbfe_tri_match_last_ms(float* ms);

/* ---- fusing a list of map points into many keyframes (ORBMatcher.fuse_pkf_mp, ORBMatcher.py:482-582) ----
 *
 * k_fuse_search, one launch for every (keyframe k, point i) of n_kf keyframes and one shared list of n_pts map
 * points: the search half of fuse_pkf_mp (:498-567).  Applying a match (:569-580) changes the map and stays with
 * the caller, in the reference's order.
 * Per keyframe: ORBFE_FUSE_KF_F64 doubles
 *   [0..4] fx fy cx cy bf   [5..13] Rcw row-major   [14..16] tcw   [17..19] Ow   [20..23] mnMinX mnMaxX mnMinY mnMaxY
 *   [24] mfGridElementWidthInv   [25] mfGridElementHeightInv   [26] mfLogScaleFactor
 * (the pose values as the keyframe's getters return them, widened exactly), three ints (grid columns, grid rows,
 * level count), n undistorted positions (x, y as doubles), n octaves, n right coordinates (negative: monocular;
 * >= 0, so also 0.0: stereo), n descriptors, one entry per level of mvScaleFactors and mvInvLevelSigma2, and the
 * grid as CSR: columns * rows + 1 offsets, cell (ix, iy) at ix * rows + iy, holding the entries of mGrid[ix][iy]
 * in the stored order.  A feature that is in no cell is never a candidate.
 * Per point: ORBFE_FUSE_PT_F64 doubles
 *   [0..2] position   [3..5] normal   [6] get_min_distance_invariance()   [7] get_max_distance_invariance()
 *   [8] mfMaxDistance
 * and its descriptor.
 * Per item, in IEEE double in this operation order without contraction (sums of three from the left):
 *   pc = Rcw p + tcw; pc.z < 0: no candidate.  invz = 1 / pc.z (pc.z == 0 gives inf, and u, v below fail the image
 *   test); u = fx * (pc.x * invz) + cx, v = fy * (pc.y * invz) + cy, ur = u - bf * invz;
 *   mnMinX <= u < mnMaxX and mnMinY <= v < mnMaxY; PO = p - Ow, dist = sqrt(PO.PO) in [min, max] distance;
 *   PO.normal >= 0.5 * dist; level = ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) clamped to [0, levels - 1];
 *   r = th * scale[level]; the cell window floor(((u - mnMinX) - r) * widthInv) .. ceil(((u - mnMinX) + r) * widthInv)
 *   (rows likewise), clamped, empty when it lies outside the grid (KeyFrame.get_features_in_area, KeyFrame.py:432-448).
 * A candidate is an entry of the window's cells, visited column by column (ix outer, iy inner, the cell's stored
 * order), with |x - u| < r and |y - v| < r, octave in [level - 1, level], and
 *   stereo: ((u - x)^2 + (v - y)^2 + (ur - right)^2) * inv_sigma2[octave] <= 7.8
 *   mono:   ((u - x)^2 + (v - y)^2) * inv_sigma2[octave] <= 5.99.
 * The candidate of the smallest Hamming distance wins, among equal distances the earliest visited.
 * Outputs at [k * out_stride + i], i < n_pts (entries past n_pts untouched): best_idx (feature index or -1),
 * best_dist (Hamming distance or -1), status.
 * The reference evaluates the same expressions in the dtypes of its operands (float32 poses and positions make the
 * whole chain float32), squares through pow and takes another library's log.  Each compared value therefore
 * carries an absolute bound on the reference's deviation, built from the magnitudes of the summed terms and
 * scaled by eps (the unit of rounding the caller chooses from its dtypes).  status gets ORBFE_FUSE_MARGINAL when
 * the bound could flip any decision taken for the item: the sign of pc.z, an image bound, the minimum or maximum
 * distance, the viewing gate, the level quotient or a window bound near an integer, a visited entry's |dx| or
 * |dy| near r, a chi-square near its threshold; also when an intermediate is not finite.  The outputs are then
 * this arithmetic's, and the caller that wants the reference's decision redoes the item with the reference's own
 * expressions.  The longest keyframe taken is ORBFE_BOW_MAX_FRAME features and as many grid entries; the point
 * count is not limited.  A workgroup takes ORBFE_FUSE_CHUNK points of one keyframe. */
#define ORBFE_FUSE_MARGINAL 1 /* status bit: a decision of the item lies within rounding of its threshold */
#define ORBFE_FUSE_KF_F64 27
#define ORBFE_FUSE_PT_F64 9
#define ORBFE_FUSE_CHUNK 256
typedef struct orbfe_fuse_out {
    int32_t* best_idx;  /* n_kf x out_stride */
    int32_t* best_dist; /* n_kf x out_stride */
    uint8_t* status;    /* n_kf x out_stride */
} orbfe_fuse_out;
/* Host buffers, synchronous.  Keyframe k is features [off[k], off[k + 1]) of xy / octave / u_right / desc32, cell
 * offsets [cell_at[k], cell_at[k + 1]) of cell_off (relative to the keyframe's first grid entry), grid entries
 * [idx_at[k], idx_at[k + 1]) of cell_idx and levels [lvl_off[k], lvl_off[k + 1]) of scale / inv_sigma2 (all four
 * offset arrays start at 0).  Everything is validated before any device call: ORBFE_EINVAL with a message for a null
 * argument, offsets that decrease, a grid whose offset count is not columns * rows + 1 or whose last offset is not
 * its entry count, a grid entry outside the keyframe's features, an octave outside the level table, a keyframe
 * above the limit, an out_stride below n_pts, a level count <= 0 or not the level tables' length, a scalar that is
 * not finite.  n_kf == 0 or n_pts == 0 launches nothing and succeeds.  Process-wide buffers, stream and events of
 * its own: concurrent callers take turns. */
int orbfe_fuse_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                      const int32_t* octave, const double* u_right, const uint8_t* desc32, const int64_t* cell_at,
                      const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                      const double* scale, const double* inv_sigma2, int32_t n_kf, const double* pt_f64,
                      const uint8_t* pt_desc32, int64_t n_pts, double th, double eps, const orbfe_fuse_out* out,
                      int64_t out_stride);
/* Kernel time of the last orbfe_fuse_search (ms, HIP events), for measurement. */
int orbfe_fuse_search_last_ms(float* ms);

/* ---- loop closing's Sim3 projection searches (ORBMatcher.fuse_kf_scw_mp, ORBMatcher.py:395-480, and
 *      ORBMatcher.search_by_projection_ckf_scw_mp, :850-922) ----
 *
 * k_scw_search, one launch for every (keyframe k, point i) of n_kf keyframes, each with a pose of its own, and one
 * shared list of n_pts map points: the search half of both functions (:409-468 and :863-916).  What is done with
 * the best candidate (:470-478, :918-920) and the TH_LOW test stay with the caller, in the reference's order.
 * The keyframe block is orbfe_fuse_search's, ORBFE_FUSE_KF_F64 doubles in the same slots, so one packing serves
 * both; slot [4] (bf) is not read and may hold anything, and the pose slots [5..19] hold Rcw, tcw and Ow as the
 * caller got them from the Sim3 (sRcw / s, t / s, -Rcw^T tcw), widened exactly.  There are no right coordinates and
 * no inverse sigma squares.  The point block and the grid are orbfe_fuse_search's.
 * Per item the arithmetic is orbfe_fuse_search's up to the cell window, without ur.  The depth gate is pc.z < 0;
 * at pc.z == 0 the division gives inf, u and v fail the image test, and the item ends without a candidate, which is
 * also what the ckf search's pc.z <= 0 gives, so one path serves both.
 * A candidate is an entry of the window's cells, visited column by column (ix outer, iy inner, the cell's stored
 * order), whose blocked byte is 0 (blocked: one byte per feature, concatenated at `off` like the octaves; NULL:
 * nothing is blocked), with |x - u| < r and |y - v| < r and octave in [level - 1, level].  There is no chi-square.
 * The candidate of the smallest Hamming distance wins, among equal distances the earliest visited.  Taking
 * candidates away never changes the order of those that remain: the winner over a smaller blocked set stands for
 * every larger one that leaves it free.
 * Outputs at [k * out_stride + i], i < n_pts (entries past n_pts untouched): best_idx (feature index or -1),
 * best_dist (Hamming distance or -1), status.  status gets ORBFE_FUSE_MARGINAL under orbfe_fuse_search's bounds,
 * scaled by eps: the sign of pc.z, an image bound, the minimum or maximum distance, the viewing gate, the level
 * quotient or a window bound near an integer, a visited entry's |dx| or |dy| near r (a blocked entry marks
 * nothing); also when an intermediate is not finite.  The limits are orbfe_fuse_search's. */
typedef struct orbfe_scw_out {
    int32_t* best_idx;  /* n_kf x out_stride */
    int32_t* best_dist; /* n_kf x out_stride */
    uint8_t* status;    /* n_kf x out_stride */
} orbfe_scw_out;
/* Host buffers, synchronous; the arrays and the checks are orbfe_fuse_search's (ORBFE_EINVAL with a message before
 * any device call; slot [4] of a keyframe block is exempt from the finiteness check), n_kf == 0 or n_pts == 0
 * launches nothing and succeeds.  Process-wide buffers, stream and events of its own: concurrent callers take
 * turns. */
int orbfe_scw_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                     const int32_t* octave, const uint8_t* desc32, const uint8_t* blocked, const int64_t* cell_at,
                     const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                     const double* scale, int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                     double th, double eps, const orbfe_scw_out* out, int64_t out_stride);
/* Kernel time of the last orbfe_scw_search (ms, HIP events), for measurement. */
int orbfe_scw_search_last_ms(float* ms);

/* ---- loop closing's mutual Sim3 search (ORBMatcher.search_by_sim3, ORBMatcher.py:713-848) ----
 *
 * k_sim3_search, one launch for n_srch searches.  A search is one direction of one keyframe pair (:742-789 or
 * :791-838): a target keyframe, a pose in two stages, and a list of map points of its own.  The mutual check and the
 * TH_HIGH test (:788, :840-846) stay with the caller.
 * The keyframes are orbfe_scw_search's arrays without `blocked`; a keyframe that several searches target appears
 * once.  Of a keyframe's ORBFE_FUSE_KF_F64 block only slots [20..26] are read (bounds, inverse cell sizes, log scale
 * factor); slots [0..19] (intrinsics, bf, pose, centre) may hold anything.  The point table is orbfe_fuse_search's,
 * ORBFE_FUSE_PT_F64 doubles and a descriptor per point; slots [3..5] (the normal) are not read and may hold anything,
 * non-finite values included.
 * Per search: ORBFE_SIM3_F64 doubles
 *   [0..3] fx fy cx cy   [4..12] Rw row-major   [13..15] tw   [16..24] sR row-major   [25..27] t
 * (the reference projects both directions with pKF1's intrinsics, so they belong to the search and not to the
 * target; sR and t as the caller got them from the Sim3 with the reference's expressions, widened exactly), the
 * index srch_kf[s] of its target keyframe, and items [srch_off[s], srch_off[s + 1]) of item_pt, each an index into
 * the point table (repeats allowed, any order).
 * Per item, in IEEE double in this operation order without contraction (sums of three from the left):
 *   c1 = Rw p + tw; c = sR c1 + t; c.z < 0: no candidate.  invz = 1 / c.z (c.z == 0 gives inf, and u, v below fail
 *   the image test); u = fx * (c.x * invz) + cx, v = fy * (c.y * invz) + cy with the search's intrinsics;
 *   mnMinX <= u < mnMaxX and mnMinY <= v < mnMaxY of the target; dist = sqrt((c.x^2 + c.y^2) + c.z^2) in [min, max]
 *   distance; there is no viewing gate; level = ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) clamped to
 *   [0, levels - 1]; r = th * scale[level]; the cell window and the candidates are orbfe_scw_search's with nothing
 *   blocked.
 * Outputs at [i], i < srch_off[n_srch], flat over the items: best_idx (feature index of the target or -1),
 * best_dist (Hamming distance or -1), status.  status gets ORBFE_FUSE_MARGINAL under orbfe_fuse_search's bounds
 * scaled by eps, carried through both stages: each component of c1 has 4 eps times the sum of its terms'
 * magnitudes, each component of c has sum_j |sR_ij| E1_j + 4 eps (sum_j |sR_ij c1_j| + |t_i|), and dist has the sum
 * of the three component bounds besides its own rounding; also when an intermediate is not finite.  The limits are
 * orbfe_fuse_search's.  A workgroup takes up to ORBFE_FUSE_CHUNK items of one search; an empty search launches
 * nothing. */
#define ORBFE_SIM3_F64 28
typedef struct orbfe_sim3_out {
    int32_t* best_idx;  /* one per item */
    int32_t* best_dist; /* one per item */
    uint8_t* status;    /* one per item */
} orbfe_sim3_out;
/* Host buffers, synchronous; the keyframe arrays and their checks are orbfe_scw_search's, except that slots [0..19]
 * of a keyframe block are exempt from the finiteness check.  Also ORBFE_EINVAL, before any device call, for a
 * srch_kf outside [0, n_kf), srch_off[0] != 0 or a srch_off that decreases, an item_pt outside [0, n_pts), a
 * srch_f64 entry that is not finite, a point scalar outside slots [3..5] that is not finite.  n_srch == 0 or
 * srch_off[n_srch] == 0 launches nothing and succeeds.  Process-wide buffers, stream and events of its own:
 * concurrent callers take turns. */
int orbfe_sim3_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                      const int32_t* octave, const uint8_t* desc32, const int64_t* cell_at, const int32_t* cell_off,
                      const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off, const double* scale,
                      int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                      const double* srch_f64, const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch,
                      const int32_t* item_pt, double th, double eps, const orbfe_sim3_out* out);
/* Kernel time of the last orbfe_sim3_search (ms, HIP events), for measurement. */
int orbfe_sim3_search_last_ms(float* ms);

/* ---- relocalisation's projection search into a frame (ORBMatcher.search_by_projection_f_kf_f,
 *      ORBMatcher.py:924-1008, with Frame.get_features_in_area, Frame.py:373-416) ----
 *
 * k_fkf_search, one launch for n_srch searches.  A search is a target frame and a list of map points of its own
 * (a keyframe's, after the caller's prefilter).  The ORBdist test, the assignment into the frame's map point slots
 * (:985-987) and the rotation histogram stay with the caller, in the reference's order; because an assignment takes
 * a feature away from the items after it, the caller redoes an item whose best feature was taken meanwhile.
 * The target arrays are orbfe_scw_search's, `blocked` included (a frame that several searches target appears once,
 * and its blocked bytes serve all of them); the point table is orbfe_fuse_search's.  The searches are
 * orbfe_sim3_search's without the search scalars: srch_kf[s] is the target, items [srch_off[s], srch_off[s + 1])
 * of item_pt index the point table (repeats allowed, any order).
 * What differs from orbfe_scw_search:
 *   - the launch is ragged and the outputs are flat over the items, as in orbfe_sim3_search; there is no out_stride;
 *   - the target is a Frame: grid columns and rows are FRAME_GRID_COLS / FRAME_GRID_ROWS, the level count and tables
 *     the frame's; the pose slots [5..16] are mTcw's rotation and translation and [17..19] Ow = -Rcw^T tcw as the
 *     caller computed it with the reference's expression, widened exactly;
 *   - there is no depth gate: pc.z < 0 goes on, so a point behind the camera whose u, v land inside the bounds is
 *     searched.  status gets ORBFE_FUSE_MARGINAL (and the item no candidate) when pc.z is 0 or within its bound of
 *     0, or when u, v or a bound of theirs is not finite;
 *   - u = (fx * pc.x) * invz + cx and v = (fy * pc.y) * invz + cy, in this order (the reference's fx * xc * invzc);
 *   - the image gate is inclusive at both ends: mnMinX <= u <= mnMaxX and mnMinY <= v <= mnMaxY;
 *   - there is no viewing gate; slots [3..5] of a point (the normal) are not read and may hold anything, non-finite
 *     values included;
 *   - both ends of the cell window truncate toward zero: trunc(((u - mnMinX) - r) * widthInv), at least 0, empty when
 *     >= columns; trunc(((u - mnMinX) + r) * widthInv), at most columns - 1, empty when negative (rows likewise).
 *     A bound in (-1, 1) is cell 0, so only a bound near an integer of magnitude >= 1 marks;
 *   - a candidate's octave lies in [level - 1, level + 1], three octaves instead of two.
 * The rest is orbfe_scw_search's: PO = p - Ow, dist = sqrt(PO.PO) in [min, max] distance, level =
 * ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) clamped to [0, levels - 1], r = th * scale[level], the visiting
 * order, |x - u| < r and |y - v| < r, a blocked entry skipped first and marking nothing, the smallest Hamming distance
 * and among equals the earliest visited, and the margins scaled by eps.
 * Outputs at [i], i < srch_off[n_srch]: best_idx (feature index of the target or -1), best_dist (Hamming distance
 * or -1), status.  The limits are orbfe_fuse_search's.  A workgroup takes up to ORBFE_FUSE_CHUNK items of one search;
 * an empty search launches nothing. */
typedef struct orbfe_fkf_out {
    int32_t* best_idx;  /* one per item */
    int32_t* best_dist; /* one per item */
    uint8_t* status;    /* one per item */
} orbfe_fkf_out;
/* Host buffers, synchronous; the target arrays and their checks are orbfe_scw_search's (slot [4] of a block is exempt
 * from the finiteness check), the searches' checks orbfe_sim3_search's: ORBFE_EINVAL, before any device call, for a
 * srch_kf outside [0, n_kf), srch_off[0] != 0 or a srch_off that decreases, an item_pt outside [0, n_pts), a point
 * scalar outside slots [3..5] that is not finite.  n_srch == 0 or srch_off[n_srch] == 0 launches nothing and succeeds.
 * Process-wide buffers, stream and events of its own: concurrent callers take turns, and none of them waits for a
 * caller of the other three searches. */
int orbfe_fkf_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                     const int32_t* octave, const uint8_t* desc32, const uint8_t* blocked, const int64_t* cell_at,
                     const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                     const double* scale, int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                     const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt,
                     double th, double eps, const orbfe_fkf_out* out);
/* Kernel time of the last orbfe_fkf_search (ms, HIP events), for measurement. */
int orbfe_fkf_search_last_ms(float* ms);

/* ---- tracking's local-map search (Tracking.search_local_points, Tracking.py:439-468: Frame.is_in_frustum,
 *      Frame.py:328-371, then ORBMatcher.search_by_projection_f_p, ORBMatcher.py:215-283) ----
 *
 * k_local_search, one launch for n_srch searches.  A search is a target frame, a limit of the viewing cosine and a
 * list of map points of its own (the local map, after the caller's prefilter).  For every item it decides what
 * is_in_frustum decides (in view or not, the predicted level) and, for an item in view, finds the best and the second
 * best candidate of search_by_projection_f_p.  The TH_HIGH test, the ratio test between the two (with the octaves of
 * best_idx and second_idx), the assignment into the frame's map point slots and the attributes is_in_frustum writes
 * stay with the caller, in the reference's order; because an assignment by a point with observations takes a feature
 * away from the items after it, the caller redoes an item whose best or second feature was taken meanwhile.
 * The target arrays are orbfe_fkf_search's, `blocked` included, plus u_right (one double per feature, concatenated at
 * `off`; <= 0: the feature has no stereo gate, the reference tests mvuRight[idx] > 0), and slot [4] of a block, bf, is
 * read.  The point table is orbfe_fuse_search's with the normal in slots [3..5], which is read.  The searches are
 * orbfe_fkf_search's plus srch_limit[s], the viewing cosine's limit (0.5 in Tracking).
 * Per item, in IEEE double in this operation order without contraction (sums of three from the left):
 *   pc = Rcw p + tcw; pc.z < 0: not in view.  invz = 1 / pc.z; u = (fx * pc.x) * invz + cx, v likewise,
 *   ur = u - bf * invz; mnMinX <= u <= mnMaxX and mnMinY <= v <= mnMaxY; PO = p - Ow, dist = sqrt(PO.PO) in [min, max]
 *   distance; view_cos = (PO.n) / dist, below srch_limit[s]: not in view; level = ceil(log(mfMaxDistance / dist) /
 *   mfLogScaleFactor) clamped to [0, levels - 1].  The item is in view.
 *   r0 = view_cos > 0.998 ? 2.5 : 4.0; r0 *= th only where th_on != 0 (the caller's th != 1.0; with th_on == 0 th is
 *   not read); r = r0 * scale[level]; the cell window is orbfe_fkf_search's, truncated at both ends.
 *   A candidate is an entry of the window's cells in orbfe_scw_search's visiting order whose blocked byte is 0, with
 *   |x - u| < r and |y - v| < r, octave in [level - 1, level], and, where u_right[f] > 0, |ur - u_right[f]| <= r.
 *   best is the candidate of the smallest key (Hamming distance, visiting position), second that of the second
 *   smallest: what the reference's sequential update (dist < best shifts best into second, else dist < best2 sets
 *   second) holds after the last candidate.
 * Outputs at [i], i < srch_off[n_srch], flat over the items: in_view (0 / 1), level (-1 when not in view), best_idx,
 * best_dist, second_idx, second_dist (-1 for none; all four -1 when not in view), status.  status gets
 * ORBFE_FUSE_MARGINAL under orbfe_fkf_search's bounds scaled by eps (the sign of pc.z, an image bound, the minimum or
 * maximum distance, the level quotient near an integer, a window bound near an integer of magnitude >= 1, a visited
 * entry's |dx| or |dy| near r; a blocked entry marks nothing) and for: view_cos within its bound of srch_limit[s] or
 * of 0.998 (the bound is 5 eps (sum of the dot product's term magnitudes) / dist + 8 eps |view_cos|, plus eps times
 * the threshold); a candidate with u_right > 0 that passed the position and octave tests whose |ur - uR| lies within
 * its bound of r (ur's bound is orbfe_fuse_search's); pc.z == 0 (the reference's NaN comparisons can let such a point
 * through its bounds); an intermediate that is not finite.  The outputs of a marked item are this arithmetic's.  The
 * limits are orbfe_fuse_search's.  A workgroup takes up to ORBFE_FUSE_CHUNK items of one search; an empty search
 * launches nothing. */
typedef struct orbfe_local_out {
    uint8_t* in_view;     /* one per item */
    int32_t* level;       /* one per item */
    int32_t* best_idx;    /* one per item */
    int32_t* best_dist;   /* one per item */
    int32_t* second_idx;  /* one per item */
    int32_t* second_dist; /* one per item */
    uint8_t* status;      /* one per item */
} orbfe_local_out;
/* Host buffers, synchronous; the target arrays and their checks are orbfe_fkf_search's, with u_right required and
 * finite where a frame has features and slot [4] of a block finite; the searches' checks are orbfe_fkf_search's, and
 * ORBFE_EINVAL, before any device call, also for a srch_limit that is not finite and for any point scalar that is not
 * finite (the normal included).  n_srch == 0 or srch_off[n_srch] == 0 launches nothing and succeeds.  Process-wide
 * buffers, stream and events of its own: concurrent callers take turns, and none of them waits for a caller of the
 * other four searches. */
int orbfe_local_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                       const int32_t* octave, const double* u_right, const uint8_t* desc32, const uint8_t* blocked,
                       const int64_t* cell_at, const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx,
                       const int64_t* lvl_off, const double* scale, int32_t n_kf, const double* pt_f64,
                       const uint8_t* pt_desc32, int64_t n_pts, const double* srch_limit, const int32_t* srch_kf,
                       const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt, double th, int32_t th_on,
                       double eps, const orbfe_local_out* out);
/* Kernel time of the last orbfe_local_search (ms, HIP events), for measurement. */
int orbfe_local_search_last_ms(float* ms);

/* ---- tracking's motion-model search (Tracking.track_with_motion_model: ORBMatcher.search_by_projection_f_f,
 *      ORBMatcher.py:291-393, with Frame.get_features_in_area, Frame.py:373-416) ----
 *
 * k_ff_search, one launch for n_srch searches.  A search is a (current frame, last frame) pair: the target is the
 * current frame, the items are the last frame's map points, each with the octave of the last frame's keypoint it was
 * seen at.  For every item it finds the best candidate among the current frame's features; the TH_HIGH test, the
 * assignment into the current frame's map point slots and the rotation histogram stay with the caller, in the
 * reference's order, and because an assignment by a point with observations takes a feature away from the items after
 * it, the caller redoes an item whose best feature was taken meanwhile.
 * The target arrays are orbfe_local_search's, u_right and `blocked` included, and slot [4] of a block, bf, is read.
 * The point table is orbfe_fuse_search's, but only the position, slots [0..2], is read: slots [3..8] may hold anything.
 * What differs from orbfe_local_search: there is no distance gate, no viewing gate and no level prediction; the level
 * is item_level[i]; th is srch_th[s], one per search (Tracking retries a pair with twice the th); the candidates'
 * octaves follow srch_mode[s]; only the best candidate comes back.
 * Per item, in IEEE double in this operation order without contraction (sums of three from the left):
 *   pc = Rcw p + tcw; pc.z < 0 (the reference's 1 / pc.z < 0): no search.  invz = 1 / pc.z; u = (fx * pc.x) * invz +
 *   cx, v likewise, ur = u - bf * invz; mnMinX <= u <= mnMaxX and mnMinY <= v <= mnMaxY; level = item_level[i];
 *   r = srch_th[s] * scale[level]; the cell window is orbfe_fkf_search's, truncated at both ends.
 *   A candidate is an entry of the window's cells in orbfe_scw_search's visiting order whose blocked byte is 0, with
 *   |x - u| < r and |y - v| < r, its octave in [level - 1, level + 1] (srch_mode[s] == 0), in [level, inf) (1: the
 *   camera moved forward) or in [0, level] (2: backward), and, where u_right[f] > 0, |ur - u_right[f]| <= r.
 *   best is the candidate of the smallest key (Hamming distance, visiting position).
 * Outputs at [i], i < srch_off[n_srch], flat over the items: best_idx, best_dist (-1 for none), status.  status gets
 * ORBFE_FUSE_MARGINAL under orbfe_local_search's bounds for what the two share (the sign of pc.z, an image bound, a
 * window bound near an integer of magnitude >= 1, a visited entry's |dx| or |dy| near r, the stereo gate near r; a
 * blocked entry marks nothing; the octave tests are integer tests) and for pc.z == 0 of either sign, which gets no
 * candidate (the reference's 1 / 0 gives inf or NaN, whose comparisons can let the point through to an int(nan) that
 * raises), and for an intermediate that is not finite.  The outputs of a marked item are this arithmetic's.  The
 * limits are orbfe_fuse_search's.  A workgroup takes up to ORBFE_FUSE_CHUNK items of one search; an empty search
 * launches nothing. */
typedef struct orbfe_ff_out {
    int32_t* best_idx;  /* one per item */
    int32_t* best_dist; /* one per item */
    uint8_t* status;    /* one per item */
} orbfe_ff_out;
/* Host buffers, synchronous; the target arrays and their checks are orbfe_local_search's; the searches' checks are
 * orbfe_fkf_search's, and ORBFE_EINVAL, before any device call, also for a srch_th that is not finite, a srch_mode
 * outside 0..2, an item_level outside [0, levels) of the item's target, and a point position that is not finite
 * (slots [3..8] are not looked at).  n_srch == 0 or srch_off[n_srch] == 0 launches nothing and succeeds.  Process-wide
 * buffers, stream and events of its own: concurrent callers take turns, and none of them waits for a caller of the
 * other five searches. */
int orbfe_ff_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                    const int32_t* octave, const double* u_right, const uint8_t* desc32, const uint8_t* blocked,
                    const int64_t* cell_at, const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx,
                    const int64_t* lvl_off, const double* scale, int32_t n_kf, const double* pt_f64,
                    const uint8_t* pt_desc32, int64_t n_pts, const double* srch_th, const int32_t* srch_mode,
                    const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt,
                    const int32_t* item_level, double eps, const orbfe_ff_out* out);
/* Kernel time of the last orbfe_ff_search (ms, HIP events), for measurement. */
int orbfe_ff_search_last_ms(float* ms);

/* ---- place recognition (KeyFrameDatabase.py, pyDBoW/ScoringObject.py) ------------------
 *
 * A database of bag-of-words vectors that stays resident on the device, and the L1 score.  A vector is
 * n distinct non-negative word ids in ascending order with one f64 weight each.  The host holds the
 * master copy: create / add / erase / clear / stats make no device call; a query first uploads what
 * the device has not seen yet.  When the slot table or the arena outgrows its capacity the capacity
 * doubles and erased vectors are dropped from the arena (regrows counts these events); slot numbers
 * of other vectors never change.
 *
 * Canonical L1 score: the terms (fabs(vi - wi) - fabs(vi)) - fabs(wi), vi the query's weight and wi the
 * stored vector's, summed in ascending word id, sequentially, in IEEE double; the score is -sum / 2.0
 * (-0.0 when no word is shared, as GeneralScoring.l1_score).  The reference sums in CPython's set
 * order; for L1-normalised vectors the two differ by at most (n_common + 3) * 2^-52. */
typedef struct orbfe_kfdb* orbfe_kfdb_handle;
/* capacity hints (>= 1): vectors and arena entries (words over all vectors) */
int orbfe_kfdb_create(int64_t kf_capacity, int64_t word_capacity, orbfe_kfdb_handle* out);
int orbfe_kfdb_destroy(orbfe_kfdb_handle h);
/* Appends one vector (n >= 0) and returns its slot; ORBFE_EINVAL unless the ids are distinct,
 * non-negative and ascending. */
int orbfe_kfdb_add(orbfe_kfdb_handle h, const int32_t* word, const double* weight, int32_t n, int64_t* slot);
/* ORBFE_EINVAL for a slot that does not exist, ORBFE_ESTATE for one already erased. */
int orbfe_kfdb_erase(orbfe_kfdb_handle h, int64_t slot);
/* Empties the database (capacities stay); slot numbers restart at 0. */
int orbfe_kfdb_clear(orbfe_kfdb_handle h);
/* Any pointer may be NULL.  n_slots counts erased slots too; live_words sums the live vectors' lengths. */
int orbfe_kfdb_stats(orbfe_kfdb_handle h, int64_t* n_slots, int64_t* n_live, int64_t* live_words,
                     int64_t* kf_capacity, int64_t* word_capacity, int64_t* regrows);
/* One launch over the whole database.  Per slot s < n_slots: common[s] = words shared with the query
 * (0 for an erased slot), first[s] = smallest shared word id (-1 when none), score[s] = canonical L1
 * score.  cap = length of the result arrays (ORBFE_ECAPACITY when below n_slots).  Host buffers,
 * synchronous. */
int orbfe_kfdb_query(orbfe_kfdb_handle h, const int32_t* q_word, const double* q_weight, int32_t nq,
                     int32_t* common, int32_t* first, double* score, int64_t cap);
/* The same kernel over n_vec vectors that are not in a database: vector v = word / weight[off[v] ..
 * off[v + 1]), off[0] = 0. */
int orbfe_bow_score(const int32_t* q_word, const double* q_weight, int32_t nq, const int64_t* off,
                    const int32_t* word, const double* weight, int32_t n_vec,
                    int32_t* common, int32_t* first, double* score);
/* Kernel time of the last orbfe_kfdb_query (ms, HIP events; 0 for an empty database). */
int orbfe_kfdb_last_ms(orbfe_kfdb_handle h, float* ms);

/* ---- many queries in one launch, gated on the device (k_bow_score_many, k_bow_gate) ----
 *
 * n_query vectors against the whole database.  Per (query q, slot s) the same common / first / score as
 * orbfe_kfdb_query gives for q alone, bit for bit.  Then, per query, the reference's word gate
 * (KeyFrameDatabase.py:60-66, 126-131) on the device:
 *   max_common[q] = the largest common over live slots that are not excluded for q (0 when there is none);
 *   n_sharing[q]  = the live slots with common > 0, excluded ones included;
 *   slot s is a hit iff it is live, not excluded for q, common > 0 and
 *                       common > (int32_t)((double)max_common[q] * gate_ratio)
 * (one IEEE double product, truncated: Python's int(max * 0.8); gate_ratio = 0 keeps every sharing slot).
 * Query q's hits are written in ascending slot order to entries [q * hit_cap, q * hit_cap + min(n_hits[q],
 * hit_cap)) of hit_slot / hit_common / hit_first / hit_score; n_hits[q] is always the true count, so
 * n_hits[q] > hit_cap tells the caller to ask again with more room.  hit_cap = 0 writes no hit (the four arrays
 * may be NULL).  Exclusions: query q's are excl_slot[excl_off[q] .. excl_off[q + 1]), ascending, distinct and
 * below n_slots (the reference's connected set; for a batch also a frame's temporal neighbours); excl_off = NULL
 * excludes nothing.  Dense rows: when common / first / score are given, row q (n_slots entries, excluded and
 * erased slots included) goes to entry q * dense_stride of each; each of the three may be NULL.
 * All buffers of *out are host memory; both entries are synchronous and run under the handle's mutex, like
 * orbfe_kfdb_query.  The dense intermediate (16 B per (query, slot)) lives in device scratch owned by the handle:
 * when it would exceed the scratch limit the queries go through the kernels in chunks, one query at the least,
 * with identical results. */
typedef struct orbfe_kfdb_many_out {
    int32_t* n_sharing;   /* [n_query]                                                     */
    int32_t* max_common;  /* [n_query]                                                     */
    int32_t* n_hits;      /* [n_query] true count, may exceed hit_cap                      */
    int32_t* hit_slot;    /* [n_query][hit_cap], ascending; entries past min(n_hits, hit_cap) unspecified */
    int32_t* hit_common;  int32_t* hit_first;  double* hit_score;   /* the same layout     */
    int32_t* common;  int32_t* first;  double* score;   /* dense [n_query][dense_stride]; each may be NULL */
} orbfe_kfdb_many_out;
/* Host queries: query q is entries [q_off[q], q_off[q + 1]) of q_word / q_weight (q_off[0] = 0, non-decreasing).
 * Everything is validated before any device call: ORBFE_EINVAL unless every query's ids are distinct,
 * non-negative and ascending, the offsets and exclusions are as above, gate_ratio lies in [0, 1) and
 * hit_cap >= 0; ORBFE_ECAPACITY when a dense array is given and dense_stride < n_slots.  n_query = 0 or an
 * empty database answers without touching the device (zeros in the three per-query arrays). */
int orbfe_kfdb_query_many(orbfe_kfdb_handle h, const int64_t* q_off, const int32_t* q_word, const double* q_weight,
                          int32_t n_query, const int64_t* excl_off, const int32_t* excl_slot, double gate_ratio,
                          int32_t hit_cap, int64_t dense_stride, const orbfe_kfdb_many_out* out);
/* Device-resident queries: query f is the n_words[f] entries from f * bow_stride of d_bow->bow_word / bow_weight
 * (device pointers), exactly what orbfe_vocab_bow_device wrote with out_stride = bow_stride; the counts are read
 * on the device and clamped to [0, bow_stride].  excl_*, *out and its arrays are host memory, checked as above.
 * The call first uploads what the device copy of the database lacks, then runs on hip_stream (void* =
 * hipStream_t), ordered after the work already enqueued there, synchronises that stream and returns with the
 * results in the host buffers.  It allocates only when the scratch has to grow. */
int orbfe_kfdb_query_many_device(orbfe_kfdb_handle h, const orbfe_bow_out* d_bow, int64_t bow_stride, int32_t n_query,
                                 const int64_t* excl_off, const int32_t* excl_slot, double gate_ratio,
                                 int32_t hit_cap, int64_t dense_stride, const orbfe_kfdb_many_out* out,
                                 void* hip_stream);
/* Upper bound in bytes (>= 0) of the dense intermediate of the many-query calls; the default is 64 MiB (4 Mi
 * (query, slot) pairs).  A chunk always holds one query at the least, so n_slots * 16 B is the floor. */
int orbfe_kfdb_set_scratch_limit(orbfe_kfdb_handle h, int64_t bytes);
/* Kernel time of the last many-query call (both kernels, summed over its chunks; ms, HIP events; 0 when the
 * call was answered without the device). */
int orbfe_kfdb_many_last_ms(orbfe_kfdb_handle h, float* ms);

#ifdef __cplusplus
}
#endif

#endif /* ORBFE_H */
