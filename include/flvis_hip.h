/* flvis_hip.h -- C ABI of the MI355X-native FLVIS hot path (libflvis_hip.so).
 *
 * Drop-in boundary for the reference's front-end tracking + local-map BA path.  Plain pointers and
 * sizes only; every function returns 0 on success or a negative flvis_status; the message of the last failure on a
 * context is available from flvis_last_error().  Nothing throws across this boundary.  The library owns all device
 * memory it allocates; pointers named d_* are DEVICE pointers supplied by the caller (HBM-resident inputs/outputs),
 * pointers named h_* are host pointers.
 *
 * Kernel-level entry points (what a maintainer binds at the reference's OpenCV call sites):
 *   flvis_hip_equalize_hist      <- cv::equalizeHist            src/frontend/f2f_tracking.cpp:127,143-144
 *   flvis_hip_pyr_down           <- pyramid level of cv::calcOpticalFlowPyrLK (buildOpticalFlowPyramid)
 *   flvis_hip_stereo_depth       <- CameraFrame::recover3DPts_c_FromStereo   src/processing/camera_frame.cpp:93-180
 *   flvis_hip_lkorb_tracking     <- LKORBTracking::tracking     src/processing/lkorb_tracking.cpp:9-202 (the whole step, one call)
 *   flvis_hip_lk_track           <- cv::calcOpticalFlowPyrLK    src/processing/lkorb_tracking.cpp:64-73,
 *                                                               src/processing/camera_frame.cpp:124-128
 *   flvis_hip_gftt               <- cv::goodFeaturesToTrack     src/processing/feature_dem.cpp:160,221
 *   flvis_hip_find_fundamental_ransac <- cv::findFundamentalMat(FM_RANSAC, 5.0, 0.99)   src/processing/lkorb_tracking.cpp:134
 *   flvis_hip_optimize_in_frame  <- OptimizeInFrame::optimize   src/processing/optimize_in_frame.cpp:10-91 (lkorb_tracking.cpp:199)
 *   flvis_hip_undistort_points   <- cv::undistortPoints(K, D, R, P)   src/processing/lkorb_tracking.cpp:87, src/frontend/f2f_tracking.cpp:301,425,
 *                                                               src/processing/camera_frame.cpp:130
 *   flvis_hip_project_points     <- cv::projectPoints           src/processing/lkorb_tracking.cpp:58, src/processing/camera_frame.cpp:116
 *   flvis_hip_feature_dem_detect / _redetect <- FeatureDEM::detect / ::redetect   src/processing/feature_dem.cpp:124-266
 *                                              (include/feature_dem.h:40-50)
 *   flvis_hip_orb_detect_and_compute / _hamming_knn2 / _orb_match  <- cv::ORB, cv::BFMatcher   src/backend/vo_loopclosing.cpp:242-243,601-639
 *   flvis_hip_bow_load_vocabulary / _set_vocabulary / _transform / _score / _score_jobs, flvis_loop_candidate
 *                                <- DBoW3::Vocabulary(file), ::transform, ::score; isLoopCandidate   vo_loopclosing.cpp:1097,249-253,417-437,520-590
 *   flvis_hip_voc_train, flvis_voc_file_save / _save_arrays   <- DBoW3::Vocabulary::create, ::save   3rdPartLib/DBow3/src/Vocabulary.cpp:142-569,1180-1256
 *   flvis_hip_lc_keyframe_landmarks(_rigs)  <- stereo LK + triangulation / depth lookup of the ORB keypoints   vo_loopclosing.cpp:255-372
 *   flvis_hip_lc_keyframe_landmarks_unrect  <- the STEREO_UNRECT case the reference leaves empty (:318-324), filled in: this project's rule
 *   flvis_hip_pnp_ransac(_rigs)  <- cv::solvePnPRansac of isLoopClosureKF                             vo_loopclosing.cpp:660-686
 *   flvis_hip_pgo_loop_closure   <- loopClosureOnCovGraphG2ONew (g2o EdgeSE3 pose graph)              vo_loopclosing.cpp:742-944
 * Pipeline-level entry points (the nodelets' work for a batch of streams / sequences):
 *   flvis_config_load, flvis_tracker_create, flvis_imu_feed, flvis_image_feed(_host), flvis_get_*   <- TrackingNodeletClass / F2FTracking
 *   flvis_ba_push_keyframe, flvis_get_correction, flvis_correction_feed                               <- LocalMapNodeletClass
 *   flvis_lc_params_load, flvis_loop_closer_*                                                          <- LoopClosingNodeletClass
 */
#ifndef FLVIS_HIP_H
#define FLVIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flvis_ctx flvis_ctx;
struct flvis_cfg; /* (defined with the pipeline-level entry points below) */

typedef enum flvis_status {
  FLVIS_OK = 0,
  FLVIS_ERR_INVALID_ARG = -1,
  FLVIS_ERR_NO_DEVICE = -2,   /* no HIP device / kernels cannot run: the product path never falls back to the CPU */
  FLVIS_ERR_HIP = -3,         /* a HIP runtime call failed (message in flvis_last_error) */
  FLVIS_ERR_CAPACITY = -4,    /* a fixed capacity (points per stream, candidates, window) would be exceeded */
  FLVIS_ERR_CONFIG = -5       /* yaml/config problem */
} flvis_status;

/* Library version string, e.g. "flvis_hip 0.1 (gfx950)". */
const char* flvis_version(void);

/* Creates a context bound to HIP device `device`.  `hip_stream` is an existing hipStream_t (e.g. torch's current
 * stream); NULL means the device's default (null) stream exactly as in HIP; FLVIS_STREAM_NEW asks the library to
 * create a private non-blocking stream.  Fails with FLVIS_ERR_NO_DEVICE when no GPU is visible. */
#define FLVIS_STREAM_NEW ((void*)(intptr_t)-1)
int flvis_hip_create(int device, void* hip_stream, flvis_ctx** out);
void flvis_hip_destroy(flvis_ctx* ctx);
const char* flvis_last_error(const flvis_ctx* ctx);
/* Blocks until all work queued on the context's stream has finished.  Then reports, once each, what the device flagged since the last
 * call: a stream join that timed out (FLVIS_ERR_HIP), a reset command that met a full keyframe queue and a local-map window past BA_LMAX /
 * BA_EMAX (FLVIS_ERR_CAPACITY, see flvis_ba_push_keyframe). */
int flvis_hip_synchronize(flvis_ctx* ctx);
/* The hipStream_t the context launches on (for event timing by the caller). */
void* flvis_hip_stream(flvis_ctx* ctx);

/* ---- kernel-level entry points; all operate on a batch of n_img independent images (one per stream) ------------ */

/* cv::equalizeHist on n_img contiguous u8 images of w x h (pitch == w, w % 4 == 0). In place allowed. */
int flvis_hip_equalize_hist(flvis_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n_img);
/* cv::cvtColor(img, gray, CV_BGR2GRAY / CV_BGRA2GRAY) as F2FTracking::image_feed applies it to 3- or 4-channel input
 * (src/frontend/f2f_tracking.cpp:74-111; mbRGB is constant 0 there): d_src [n_img][h][w][channels] interleaved,
 * d_dst [n_img][h][w].  w % 4 == 0. */
int flvis_hip_cvt_bgr_to_gray(flvis_ctx* ctx, const uint8_t* d_src, int channels, uint8_t* d_dst, int w, int h, int n_img);

/* cv::pyrDown (5-tap Gaussian, REFLECT_101, (x+128)>>8): n_img images w x h (pitch src_pitch) ->
 * ((w+1)/2) x ((h+1)/2) images with pitch dst_pitch.  Image i starts at d_src + i*src_pitch*h (resp. dst). */
int flvis_hip_pyr_down(flvis_ctx* ctx, const uint8_t* d_src, int w, int h, int src_pitch, uint8_t* d_dst,
                       int dst_pitch, int n_img);

/* cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(31,31), max_level,
 *                          TermCriteria(COUNT+EPS, max_iter, eps), use_initial_flow ? OPTFLOW_USE_INITIAL_FLOW : 0)
 * for n_img image pairs at once.  d_prev/d_next: [n_img][h][w] u8, tightly packed, any w >= 32 (rows that are not dword aligned, e.g.
 * KITTI's 1241, are first copied into a pitch-aligned level 0).  Points: d_prev_pts/d_next_pts [n_img][nmax][2]
 * float (x,y); d_next_pts is in/out; d_status [n_img][nmax] u8; d_count [n_img] int = valid points per image.
 * Pyramids are built internally (as OpenCV does for raw Mats). */
int flvis_hip_lk_track(flvis_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_next, int w, int h, int n_img,
                       const float* d_prev_pts, float* d_next_pts, uint8_t* d_status, const int* d_count, int nmax,
                       int max_level, int max_iter, double eps, int use_initial_flow);

/* cv::goodFeaturesToTrack(img, corners, max_corners, quality, min_distance) (blockSize 3, min-eigenvalue).
 * d_out_xy [n_img][max_corners][2] float, d_out_count [n_img] int. */
int flvis_hip_gftt(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img, int max_corners, double quality,
                   double min_distance, float* d_out_xy, int* d_out_count);

/* FeatureDEM::detect(img, newPts) with FeatureDEM(w, h, f_para) (f_para = feature_para1..6 of the yaml).
 * d_out_xy [n_img][out_cap][2] float, d_out_count [n_img]. */
int flvis_hip_feature_dem_detect(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img, const double* f_para,
                                 float* d_out_xy, int* d_out_count, int out_cap);

/* FeatureDEM::redetect(img, existedPts, newPts, n): d_exist_xy [n_img][exist_cap][2] double, d_exist_count [n_img]. */
int flvis_hip_feature_dem_redetect(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img, const double* f_para,
                                   const double* d_exist_xy, const int* d_exist_count, int exist_cap, float* d_out_xy,
                                   int* d_out_count, int out_cap);

/* ---- ORB extraction + Hamming matching: the keyframe-rate front half of the reference's loop closing.
 * Replaces cv::ORB::create(nfeatures, scaleFactor, nlevels, 31, 0, 2, cv::ORB::HARRIS_SCORE, 31, fastThreshold)
 *            ->detectAndCompute(img0, cv::Mat(), keypoints, descriptors)        src/backend/vo_loopclosing.cpp:242-243
 * (edgeThreshold 31, firstLevel 0, WTA_K 2, HARRIS_SCORE, patchSize 31 are the only values the reference uses and are
 * fixed here).  Batched over n_img images of one size.  Keypoints come out level-major, raster order within a level
 * (OpenCV's order is an artefact of std::nth_element); d_kps rows are (x, y, size, angle_deg, response, octave).
 * h_pattern: host table of the 256 test pairs as int8 [512][2] (x, y), e.g. OpenCV's learned bit_pattern_31_ when the
 * descriptors must be compatible with a DBoW vocabulary; NULL selects OpenCV's generator makeRandomPattern(31, ., 512)
 * (flvis_orb_default_pattern).  d_overflow (optional, [n_img]) is set non-zero where a capacity truncated the result.
 *
 * Capacities and what survives them.  Both retainBest cuts keep, as OpenCV does, everything >= the n-th best, so a class of equal
 * scores / equal Harris responses (integer sums: periodic imagery ties exactly) that straddles a cut is kept whole and a level can
 * return more than its budget nfeat[l] (orb.cpp's geometric split of nfeatures).  Three capacities bound that, each per image:
 *   1. candidates: at most 8192 survivors of the FAST-score cut (>= the (2 nfeat[l])-th best score) per level.  Beyond that the
 *      first 8192 in raster order go on, and the Harris cut of that level is taken among them alone: the level's list is then
 *      some valid keypoints of the level, not necessarily a prefix of the untruncated list.
 *   2. per level: at most lvl_cap = m + m / 4 + 64 keypoints with m = max_l nfeat[l] (335 for the reference's parameters).  The
 *      Harris threshold is still the one over all candidates; the first lvl_cap keypoints >= it in raster order survive.
 *   3. the caller's cap: of the level-major concatenation of the level lists the first cap rows survive, d_count = min(total, cap).
 * Every truncation sets d_overflow of its image (the flags of all n_img images are cleared at the start of each call) and
 * touches nothing else: the other images of the batch, the levels that did not overflow, and the rows [d_count, cap) of d_kps /
 * d_desc, which are never written.  Without truncation the result is complete and d_overflow is 0.
 * Refused before anything is launched or written: w or h < 64 or > 32767, nlevels outside 1 .. 12, scale_factor <= 1,
 * nfeatures < 1, fast_threshold outside 1 .. 254, a level smaller than 8 px (FLVIS_ERR_INVALID_ARG), and 2 m > 6144
 * (FLVIS_ERR_CAPACITY: the candidate buffer must hold retainBest(2 m) with room for ties).  A level of 62 px or less in either
 * direction has no border box and yields no keypoints.
 * flvis_loop_closer calls this with nfeatures 1000 and cap 1024 and does not read the flag: a keyframe with more than 1024
 * keypoints (ties make that possible) is stored from its first 1024 rows, silently. */
typedef struct flvis_orb_params {
  int nfeatures;       /* 1000 in the reference */
  float scale_factor;  /* 1.2f */
  int nlevels;         /* 8 (<= 12) */
  int fast_threshold;  /* 20 */
} flvis_orb_params;
int flvis_hip_orb_detect_and_compute(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img,
                                     const flvis_orb_params* prm, const int8_t* h_pattern, float* d_kps, uint8_t* d_desc,
                                     int* d_count, int cap, int* d_overflow);
int flvis_orb_default_pattern(int8_t* h_pattern512x2);
/* building blocks at their OpenCV call shapes (device pointers, [n_img] images, tightly packed):
 * cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR); the FAST-9/16 score map (0 = not a corner) behind
 * cv::FAST(img, kps, threshold, true); cv::GaussianBlur(src, dst, Size(7,7), 2, 2, BORDER_REFLECT_101). */
int flvis_hip_resize_linear(flvis_ctx* ctx, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, int n_img);
int flvis_hip_fast_score(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img, int threshold, uint8_t* d_score);
int flvis_hip_gaussian_blur7(flvis_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n_img);
/* cv::BFMatcher(cv::NORM_HAMMING, false).knnMatch(query, train, matches, 2) (vo_loopclosing.cpp:601-613) for n_pairs
 * independent (query, train) sets of 32-byte descriptors: d_query [n_pairs][qcap][32], d_nq [n_pairs], likewise train.
 * d_idx / d_dist: [n_pairs][qcap][2], ascending distance, ties keep the lower train index; -1 / INT_MAX when absent.
 * A count above its capacity is read as the capacity, a negative one as 0; rows [count, qcap) of d_idx / d_dist are not written. */
int flvis_hip_hamming_knn2(flvis_ctx* ctx, const uint8_t* d_query, const int* d_nq, int qcap, const uint8_t* d_train,
                           const int* d_nt, int tcap, int n_pairs, int* d_idx, int* d_dist);
/* the mutual-best + ratio test of vo_loopclosing.cpp:603-639 (knnMatch both ways, keep i when the best match of its best
 * match is i and d0/d1 < ratio_max), pairs (index in a, index in b) in ascending a order: d_pairs [n_pairs][acap][2].
 * Counts are clamped as in flvis_hip_hamming_knn2; a set of fewer than 2 descriptors gives no pair (knnMatch has no second
 * neighbour), and so does d0 = d1 = 0 (exact duplicates in b: 0/0 is not < ratio_max).  Rows [d_npairs, acap) are not written. */
int flvis_hip_orb_match(flvis_ctx* ctx, const uint8_t* d_a, const int* d_na, int acap, const uint8_t* d_b, const int* d_nb,
                        int bcap, int n_pairs, double ratio_max, int* d_pairs, int* d_npairs);

/* ---- place recognition of the loop closing: DBoW3 bag of words + L1 score + candidate selection ---------------
 * The vocabulary is handed over as flat arrays (the reference loads a DBoW3 file that is not shipped with it,
 * vo_loopclosing.cpp:1097): node 0 is the root, the children of node n are h_child_idx[h_child_ptr[n] .. h_child_ptr[n+1]) in
 * DBoW3's order (3rdPartLib/DBow3/src/Vocabulary.h m_nodes[n].children), a node without children is a word with id h_word_id[n]
 * and weight h_weight[n] (idf), no two words with the same id; h_desc: 32 bytes per node.  Weighting TF_IDF, scoring L1_NORM (DBoW3's
 * defaults). */
int flvis_hip_bow_set_vocabulary(flvis_ctx* ctx, int n_nodes, const int* h_child_ptr, const int* h_child_idx, const uint8_t* h_desc,
                                 const double* h_weight, const int* h_word_id);
/* `Vocabulary vocTmp(vocFile)` (vo_loopclosing.cpp:1095-1099; Vocabulary::load, 3rdPartLib/DBow3/src/Vocabulary.cpp:1082-1096):
 * reads a DBoW3 vocabulary file -- binary .dbow3 (plain or QuickLZ-compressed, Vocabulary.cpp:1335-1407), ORB-SLAM2 style .txt
 * (:1259-1332) or OpenCV FileStorage yaml / yaml.gz (:1411-1462) -- and makes it the context's vocabulary.  ORB vocabularies
 * (32-byte CV_8U descriptors) with weighting TF_IDF or TF and scoring L1_NORM; anything else fails with FLVIS_ERR_CONFIG. */
int flvis_hip_bow_load_vocabulary(flvis_ctx* ctx, const char* path);
/* the file reader on its own (host only, no device needed): the flat arrays flvis_hip_bow_set_vocabulary takes, owned by the
 * handle until flvis_voc_file_close.  info8 = {n_nodes, n_words, k, L, scoringType, weightingType, n_edges, layout}, layout
 * 0 binary, 1 binary QuickLZ, 2 text, 3 yaml, 4 trained by flvis_hip_voc_train (not from a file).  word_id is -1 on inner nodes. */
typedef struct flvis_voc_file flvis_voc_file;
int flvis_voc_file_open(const char* path, flvis_voc_file** out, char* err, int errlen);
int flvis_voc_file_info(const flvis_voc_file* voc, int* info8);
int flvis_voc_file_arrays(const flvis_voc_file* voc, const int** child_ptr, const int** child_idx, const uint8_t** desc,
                          const double** weight, const int** word_id);
void flvis_voc_file_close(flvis_voc_file* voc);
/* Vocabulary::save for the binary layout (host only): layout 0 writes the uncompressed .dbow3 stream of Vocabulary::toStream(out,
 * false) (Vocabulary.cpp:1180-1256), byte for byte; layouts 1 .. 3 (QuickLZ, text, yaml) have no writer and return
 * FLVIS_ERR_INVALID_ARG, as do null arguments and links that do not form a tree below node 0; FLVIS_ERR_CONFIG when the file cannot
 * be written.  flvis_voc_file_save takes any handle -- trained, or opened from any readable layout, which makes it the converter
 * to .dbow3 --, flvis_voc_file_save_arrays the flat arrays themselves (word_id is read on the leaves only). */
int flvis_voc_file_save(const flvis_voc_file* voc, const char* path, int layout);
int flvis_voc_file_save_arrays(const char* path, int layout, int n_nodes, const int* child_ptr, const int* child_idx,
                               const uint8_t* desc, const double* weight, const int* word_id, int k, int L, int scoring,
                               int weighting);
/* Vocabulary::create (3rdPartLib/DBow3/src/Vocabulary.cpp:142-569) on the device, for the descriptors this library's ORB extractor
 * leaves in d_desc [n_img][cap][32] / d_count [n_img] (a count above cap reads as cap, a negative one as 0; an image without
 * descriptors still counts as a document): hierarchical k-means with k-means++ seeding and bit-majority means, then the idf
 * weights from every training descriptor sent down the finished tree.  Two departures from DBoW3: each
 * split node draws from its own glibc stream srand(seed + node id) and nodes are numbered breadth-first (so L = 1 is exactly
 * Vocabulary::create after srand(seed)); a node's k-means ends after max_iters association passes.  Integer arithmetic throughout:
 * two runs give the same tree bit for bit, whatever small_node_max.
 * *out: a handle as flvis_voc_file_open returns it (info8.layout = 4), to be passed to flvis_voc_file_arrays / _save / _close.
 * stats8 (may be null) = {descriptors, nodes, words, association passes in total, nodes that hit max_iters, children created
 * without a descriptor (empty clusters kept), nodes split trivially (n <= k), kernel launches}.
 * FLVIS_ERR_INVALID_ARG, before anything is launched: null pointers, k outside 2 .. 64, L outside 1 .. 10, weighting other than
 * 0 / 1, max_iters or small_node_max negative, cap <= 0 or > 2048, n_img <= 0, no descriptor at all.
 * FLVIS_ERR_CAPACITY, also before anything is launched: more than 65535 images, or more than 2^25 (33 554 432) descriptors. */
typedef struct flvis_voc_train_params {
  int k, L;           /* branching factor 2 .. 64, depth 1 .. 10 */
  int weighting;      /* 0 TF_IDF, 1 TF (every word weight 1) */
  unsigned seed;
  int max_iters;      /* association passes per node; 0 = 100 */
  int small_node_max; /* nodes of at most this many descriptors are clustered by one workgroup in LDS; 0 = 2048; values above what
                         LDS holds are clamped */
} flvis_voc_train_params;
int flvis_hip_voc_train(flvis_ctx* ctx, const uint8_t* d_desc, const int* d_count, int cap, int n_img,
                        const flvis_voc_train_params* params, flvis_voc_file** out, int64_t* stats8);
/* voc.transform(kf.lm_descriptor, kf_bv) (vo_loopclosing.cpp:249-253; Vocabulary.cpp:628-688) for n_img keyframes:
 * d_desc [n_img][dcap][32] + d_count [n_img] as flvis_hip_orb_detect_and_compute leaves them (dcap <= 2048);
 * out: d_ids / d_vals [n_img][vcap] ascending word ids and L1-normalised values, d_nnz [n_img]; vcap >= min(dcap, words of the
 * vocabulary), so that no vector is ever truncated. */
int flvis_hip_bow_transform(flvis_ctx* ctx, const uint8_t* d_desc, const int* d_count, int dcap, int n_img, int vcap, int* d_ids,
                            double* d_vals, int* d_nnz);
/* STEP 1.5 / 1.6 of the loop-closing keyframe (vo_loopclosing.cpp:255-372) for n_img keyframes: the 3-D position of every ORB
 * keypoint and the lists without the keypoints that have none.  cam_type as flvis_cfg.cam_type: 0 STEREO_RECT -- d_img0 / d_img1
 * [n_img][h][w] mono8, calcOpticalFlowPyrLK(Size(31,31), 5, 30 / 0.001, USE_INITIAL_FLOW) from the keypoints into img1 (:274-278),
 * then Triangulation::trignaulationPtFromStereo with the rectified 3x4 projections h_P0 / h_P1 (row-major; range 100);
 * 2 DEPTH_D435 -- d_img1 [n_img][h][w] Z16, d = Z16 / 1000 as the INTEGER division the reference writes (:331), kept when
 * 0.3 <= d <= 10, back-projected with h_K4 = fx, fy, cx, cy (d_img0 unused); 1 STEREO_UNRECT -- the reference's case is empty,
 * every count is 0.  d_kps [n_img][cap][6] / d_desc [n_img][cap][32] / d_count as flvis_hip_orb_detect_and_compute leaves them
 * (cap <= 2048).  Out, order kept: d_lm_2d [n_img][cap][2] float, d_lm_3d [n_img][cap][3] double (camera frame), d_lm_desc
 * [n_img][cap][32] (may alias d_desc), d_lm_count [n_img]. */
int flvis_hip_lc_keyframe_landmarks(flvis_ctx* ctx, const uint8_t* d_img0, const void* d_img1, int w, int h, int n_img, int cam_type,
                                    const double* h_P0, const double* h_P1, const double* h_K4, const float* d_kps, const uint8_t* d_desc,
                                    const int* d_count, int cap, float* d_lm_2d, double* d_lm_3d, uint8_t* d_lm_desc, int* d_lm_count);
/* as flvis_hip_lc_keyframe_landmarks with one camera per image: h_P0 / h_P1 [n_img][12] (cam_type 0), h_K4 [n_img][4] (cam_type 2).  Image i
 * gets bit for bit what the call above gives it alone with row i; w, h and cam_type hold for the whole call.  The host arrays may be freed
 * when the call returns. */
int flvis_hip_lc_keyframe_landmarks_rigs(flvis_ctx* ctx, const uint8_t* d_img0, const void* d_img1, int w, int h, int n_img, int cam_type,
                                         const double* h_P0, const double* h_P1, const double* h_K4, const float* d_kps, const uint8_t* d_desc,
                                         const int* d_count, int cap, float* d_lm_2d, double* d_lm_3d, uint8_t* d_lm_desc, int* d_lm_count);
/* The STEREO_UNRECT case (the EuRoC camera), which the reference leaves as three comments -- "track to another image / go to undistor
 * plane / triangulation" -- and a break (vo_loopclosing.cpp:318-324).  The two calls above keep that empty case (every count 0); this
 * one fills it in, as an addition of this project: the STEREO_RECT case with the tracker's undistortion in front of the DLT
 * (CameraFrame::recover3DPts_c_FromStereo, camera_frame.cpp:124-147).  Per keypoint (x, y) of the RAW img0: the match in the RAW img1 by
 * calcOpticalFlowPyrLK(Size(31,31), 5, 30 / 0.001, USE_INITIAL_FLOW) seeded at the same pixel; where its status is 1,
 * u0 = undistortPoints((x, y), K0, D0, R0, P0), u1 = undistortPoints(match, K1, D1, R1, P1) (Point2f, as OpenCV returns them) and
 * pc = Triangulation::triangulationPt(u0, u1, P0, P1); kept unless pc.z < 0 or pc.z > 100.
 * Out, order kept: d_lm_2d = u0, the pixel in the RECTIFIED plane (where K = P0[0], P0[5], P0[2], P0[6] without distortion -- the K of
 * the pair check's solvePnPRansac -- holds); d_lm_3d = pc in the RECTIFIED camera-0 frame (the frame of the tracker's T_c_w on this rig);
 * the descriptor.  Outputs, aliasing (d_lm_desc == d_desc), count clamping and "rows from d_lm_count on are never written" are those of
 * flvis_hip_lc_keyframe_landmarks; cap <= 2048.
 * h_cfgs: finalized configs (flvis_config_load), read during the call (they may be freed on return): K, D of both cameras, R0 / R1 /
 * P0 / P1.  n_cfgs = 1: one rig for every image; n_cfgs = n_img: one per image, and image i gets bit for bit what the call gives it alone
 * with h_cfgs[i].
 * Refused before anything is launched or written: a config whose cam_type is not 1 or whose image size is not w x h
 * (FLVIS_ERR_CONFIG); n_cfgs other than 1 or n_img, null pointers (FLVIS_ERR_INVALID_ARG); cap > 2048 (FLVIS_ERR_CAPACITY). */
int flvis_hip_lc_keyframe_landmarks_unrect(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, int w, int h, int n_img,
                                           const struct flvis_cfg* h_cfgs, int n_cfgs /* 1: one rig for every image; n_img: one per image */,
                                           const float* d_kps, const uint8_t* d_desc, const int* d_count, int cap, float* d_lm_2d,
                                           double* d_lm_3d, uint8_t* d_lm_desc, int* d_lm_count);
/* one row of the similarity matrix (vo_loopclosing.cpp:417-437): voc.score(query, db[j]) for j < n_db (ScoringObject.cpp:23-68);
 * the query is one vector on the device (d_q_nnz[0] entries), the database [n_db][vcap]; d_db_nnz[j] < 0 marks an absent keyframe
 * (kf_lc_tmp[j] == nullptr: score 0). */
int flvis_hip_bow_score(flvis_ctx* ctx, const int* d_q_ids, const double* d_q_vals, const int* d_q_nnz, const int* d_db_ids,
                        const double* d_db_vals, const int* d_db_nnz, int vcap, int n_db, double* d_scores);
/* several rows in one launch over ONE store of vectors (d_ids / d_vals [n_vectors][vcap], d_nnz [n_vectors]): job i = h_jobs3[3i..3i+2]
 * = (query vector, first database vector, number of database vectors); d_scores[first + j] = score(query, first + j).  The loop
 * closer's rows of all sequences that got a keyframe.  At most 65535 jobs. */
int flvis_hip_bow_score_jobs(flvis_ctx* ctx, int n_jobs, const int* h_jobs3, const int* d_ids, const double* d_vals, const int* d_nnz, int vcap,
                             double* d_scores);
/* the same with an output position per job: job i = h_jobs4[4i..4i+3] = (query vector, first database vector, number of database vectors,
 * first output index); d_scores[out + j] = score(query, first + j), flvis_hip_bow_score's value bit for bit.  Two queries may score the
 * same database range, each into a row of its own: what flvis_loop_closer_localize_in needs.  At most 65535 jobs. */
int flvis_hip_bow_score_jobs_at(flvis_ctx* ctx, int n_jobs, const int* h_jobs4, const int* d_ids, const double* d_vals, const int* d_nnz, int vcap,
                                double* d_scores);
/* The candidate choice of flvis_loop_closer_localize_in.  A score row is cut into n_seg segments of seg_len entries (the closer: one segment
 * per sequence's map), of which the first d_seg_n[s] count and the rest is never read.  Per query q: the n_best (1 .. 8) entries with the
 * highest score among those with score > 0 and score >= min_score (a NaN is never picked), in segment d_map[q] or, with d_map[q] = -1, in
 * all segments; score descending, equal scores by global index s * seg_len + j ascending.  d_idx [n_q][n_best]: the global index, -1 for
 * an empty rank; d_score: the entry's score, 0 there; d_count [n_q]: the ranks filled.  n_seg * seg_len < 2^31. */
int flvis_hip_lc_select_maps(flvis_ctx* ctx, int n_q, const double* d_scores /* [n_q][n_seg * seg_len] */, int n_seg, int seg_len,
                             const int* d_seg_n, const int* d_map, int n_best, double min_score, int* d_idx, double* d_score, int* d_count);
/* flvis_hip_lc_select_maps with an excluded range per query, the candidate choice of flvis_loop_closer_link: d_skip [n_q][2] = (lo, hi), and
 * the global indices lo <= s * seg_len + j < hi are never candidates of query q, whatever bits the row holds there (NaN, stale scores,
 * memory never written: those entries are not read).  lo >= hi excludes nothing, and the result is then flvis_hip_lc_select_maps' bit for
 * bit.  Order, predicate, tie rule, empty ranks and counts are that call's. */
int flvis_hip_lc_select_maps_skip(flvis_ctx* ctx, int n_q, const double* d_scores /* [n_q][n_seg * seg_len] */, int n_seg, int seg_len,
                                  const int* d_seg_n, const int* d_map, const int* d_skip /* [n_q][2] */, int n_best, double min_score,
                                  int* d_idx, double* d_score, int* d_count);
/* ... on the closer's compact rows, the layout of a call in which no query searches all maps: d_scores [n_q][seg_len] holds segment d_map[q]
 * alone (every d_map[q] in 0 .. n_seg - 1; the caller sees to that).  Indices reported, and d_skip, are global as above.  d_skip may be NULL: no
 * range. */
int flvis_hip_lc_select_maps_skip_compact(flvis_ctx* ctx, int n_q, const double* d_scores /* [n_q][seg_len] */, int n_seg, int seg_len,
                                          const int* d_seg_n, const int* d_map, const int* d_skip, int n_best, double min_score, int* d_idx,
                                          double* d_score, int* d_count);
/* isLoopCandidate (vo_loopclosing.cpp:520-590) on the newest keyframe's row h_row[i] = sim_matrix[i][g_size-1] (host control
 * logic, as in the reference's pgoProcess thread).  Returns 1 and *kf_prev_idx when there is a candidate, 0 when not. */
int flvis_loop_candidate(int g_size, const double* h_row, const uint8_t* h_present, int lcKFDist, int lcKFMaxDist, int lcNKFClosest,
                         double minScore, int64_t* kf_prev_idx);
/* the geometric check of isLoopClosureKF (vo_loopclosing.cpp:660-686): cv::solvePnPRansac(p3d, p2d, K, Mat(), r, t, false,
 * iterations = 100, reprojectionError = 2.0, confidence = 0.99, inliers, SOLVEPNP_P3P) for n_sets independent correspondence sets
 * (one workgroup each): d_p3d [n_sets][cap][3] / d_p2d [n_sets][cap][2] float (what the reference casts to), d_count [n_sets]
 * (cap <= 1024), h_K4 = fx fy cx cy, h_seeds: one 64-bit seed of the sample generator per set.  Out: d_pose7 [n_sets][7]
 * (tx ty tz qx qy qz qw of T_c_w; identity when no model was found), d_inlier_mask [n_sets][cap], d_n_inliers [n_sets] (the caller
 * applies the acceptance rule of :677-686).  The tracker's solver on caller arrays, cv::solvePnPRansac's structure: 4-point subsets from
 * cv::RNG((uint64)-1) in getSubset's order (h_seeds is accepted and ignored: OpenCV seeds every run the same), P3P hypotheses (three
 * points, the fourth picks among the solutions), RANSACUpdateNumIters, and the final solvePnP(SOLVEPNP_EPNP) on the inliers (DESIGN.md
 * section 2 lists what is restated and what cannot be bitwise OpenCV's). */
int flvis_hip_pnp_ransac(flvis_ctx* ctx, const float* d_p3d, const float* d_p2d, const int* d_count, int cap, int n_sets, const double* h_K4,
                         int iterations, double reproj_px, double confidence, const uint64_t* h_seeds, double* d_pose7,
                         uint8_t* d_inlier_mask, int* d_n_inliers);
/* as flvis_hip_pnp_ransac with one camera per set: h_K4 [n_sets][4]; set i gets bit for bit what the call above gives it alone with row i.
 * The host arrays may be freed when the call returns. */
int flvis_hip_pnp_ransac_rigs(flvis_ctx* ctx, const float* d_p3d, const float* d_p2d, const int* d_count, int cap, int n_sets,
                              const double* h_K4, int iterations, double reproj_px, double confidence, const uint64_t* h_seeds,
                              double* d_pose7, uint8_t* d_inlier_mask, int* d_n_inliers);
/* Test hook: cv::solvePnP(..., SOLVEPNP_EPNP) alone (the solver inside flvis_hip_pnp_ransac and the tracker's PnP RANSAC) on n_sets
 * correspondence sets laid out as for flvis_hip_pnp_ransac (d_count[i] >= 4 points each), one wavefront per set.  d_out160 [n_sets][160]:
 * R (9, row-major) t (3) ok (1) | betas of the three approximations (12) | their mean reprojection errors (3) | the four eigenvectors of
 * MtM (48) | L (60) | rho (6) | the eigenvalues of MtM (12) | unused (6). */
int flvis_hip_debug_epnp(flvis_ctx* ctx, const float* d_p3d, const float* d_p2d, const int* d_count, int cap, int n_sets, const double* h_K4,
                         double* d_out160);
/* Test hook: the tracker's branch of the same solver on caller arrays -- cv::solvePnPRansac(..., SOLVEPNP_ITERATIVE) as
 * LKORBTracking::tracking calls it (lkorb_tracking.cpp:170-177, there with iterations = 100, reprojectionError = 3.0, confidence = 0.99):
 * 5-point subsets, EPnP hypotheses, Gauss-Newton on the winning model's inliers.  Arguments as for flvis_hip_pnp_ransac, with h_guess7
 * [n_sets][7] (tx ty tz qx qy qz qw, unit quaternion) in place of the seeds: the pose a set gets back when no model is found (as a
 * rotation matrix turned into a quaternion again), with n_inliers 0 and an all-zero mask.  The host arrays may be freed when the call
 * returns. */
int flvis_hip_debug_pnp_ransac_iterative(flvis_ctx* ctx, const float* d_p3d, const float* d_p2d, const int* d_count, int cap, int n_sets,
                                         const double* h_K4, int iterations, double reproj_px, double confidence,
                                         const double* h_guess7 /* [n_sets][7] */, double* d_pose7, uint8_t* d_inlier_mask, int* d_n_inliers);
/* ---- the solver calls of LKORBTracking::tracking (lkorb_tracking.cpp:9-202) and OptimizeInFrame::optimize on caller arrays ----
 * Common to the four calls below: they are batched over n_sets independent sets (a set is one frame, as in flvis_hip_stereo_depth), arrays
 * are [n_sets][cap]..., and they work on the context's stream.  d_count [n_sets]: a count above cap reads as cap, a negative one as 0;
 * rows from the count on are never written.  Argument errors (a null pointer, cap <= 0, n_sets <= 0, what each call names) are refused
 * before anything is launched or written.  The host arrays may be freed when the call returns.
 *
 * cv::findFundamentalMat(m1, m2, FM_RANSAC, thr_px, confidence, mask) (lkorb_tracking.cpp:134: 5.0, 0.99) -- the mask only, which is
 * all the reference uses.  d_m1 / d_m2 [n_sets][cap][2] float (cv::Point2f), d_mask [n_sets][cap], d_n_inliers [n_sets] = the ones of
 * each set's mask.  OpenCV's dispatch: fewer than 7 points give an all-zero mask, exactly 7 all ones, 8 .. 14 the LMedS registrator, from
 * 15 on the RANSAC registrator (1000 iterations at most); both draw their 7-point subsets from cv::RNG((uint64)-1) in getSubset's order
 * with FMEstimatorCallback::checkSubset, so a set's mask is a function of its points alone.  The tracker's own search on caller arrays.
 * FLVIS_ERR_CAPACITY for cap > 1024; FLVIS_ERR_INVALID_ARG for thr_px <= 0 or confidence outside (0, 1). */
int flvis_hip_find_fundamental_ransac(flvis_ctx* ctx, const float* d_m1, const float* d_m2, const int* d_count, int cap, int n_sets,
                                      double thr_px, double confidence, uint8_t* d_mask, int* d_n_inliers);
/* OptimizeInFrame::optimize (optimize_in_frame.cpp:10-91): g2o Levenberg on one free pose over EdgeSE3ProjectXYZOnlyPose edges with
 * Huber(1).  Inputs are the arrays getValidInliersPair hands the reference: d_lm_3d_w [n_sets][cap][3], d_lm_2d_undistort [n_sets][cap][2],
 * d_lm_id [n_sets][cap] (the edge ids); h_K4 fx fy cx cy, [n_K][4] with n_K = 1 (every set) or n_sets (one camera per set); d_pose7
 * [n_sets][7] T_c_w as tx ty tz qx qy qz qw, in / out; d_ok [n_sets].  Fewer than 10 edges: ok = 0, the pose untouched.  Otherwise the
 * active edges are taken in ascending id, equal ids in input order; two iterations; edges with chi2 > 3 are dropped; fewer than 10 left:
 * ok = 0, the pose untouched; two more iterations, the pose written, ok = 1.
 * FLVIS_ERR_CAPACITY for cap > 512 (the batched tracker truncates a frame there; a call refuses). */
int flvis_hip_optimize_in_frame(flvis_ctx* ctx, const double* d_lm_3d_w, const double* d_lm_2d_undistort, const int64_t* d_lm_id,
                                const int* d_count, int cap, int n_sets, const double* h_K4, int n_K /* 1 or n_sets */,
                                double* d_pose7 /* in/out */, uint8_t* d_ok);
/* cv::undistortPoints(src, dst, K, D, R, P) (k1 k2 p1 p2, five iterations) and cv::projectPoints(p3d, rvec(T), tvec(T), K, D, dst), one
 * thread per point: d_src / d_dst [n_sets][cap][2] float, d_p3d [n_sets][cap][3] float.  h_K4 / h_D4 / h_R9 / h_P12 (row-major 3x3 and
 * 3x4): [n_cam][...] with n_cam = 1 (every set) or n_sets; h_pose7 [n_sets][7] (tx ty tz qx qy qz qw) the pose each set is projected with.
 * A point at z = 0 is projected with 1 / z taken as 1, as OpenCV does.  n_sets <= 65535. */
int flvis_hip_undistort_points(flvis_ctx* ctx, const float* d_src, const int* d_count, int cap, int n_sets, const double* h_K4,
                               const double* h_D4, const double* h_R9, const double* h_P12, int n_cam /* 1 or n_sets */, float* d_dst);
int flvis_hip_project_points(flvis_ctx* ctx, const float* d_p3d, const int* d_count, int cap, int n_sets,
                             const double* h_pose7 /* [n_sets][7] */, const double* h_K4, const double* h_D4, int n_cam, float* d_dst);
/* loopClosureOnCovGraphG2ONew (vo_loopclosing.cpp:742-944) for n_graphs independent sequences in one launch (one workgroup per
 * pose graph): graph g has h_n_kf[g] keyframes with T_c_w (device, 7 doubles each: tx ty tz qx qy qz qw, graphs concatenated, in/out)
 * and presence flags (host, concatenated; 0 = kf_map_lc[i] == nullptr), h_n_loops[g] recorded loops (host ids: earlier, later
 * keyframe; device poses: the verified T_later_earlier the reference keeps in loop_poses).  Vertices kf_prev..kf_curr, EdgeSE3 to
 * the next five keyframes + one per loop, information I, Cauchy kernel, Levenberg with lambda 1e-10, `iterations` (100 in the
 * reference); use_initial_guess = optimizer.computeInitialGuess() (:883).  Out: the optimised keyframes' T_c_w in place,
 * d_drift7 [n_graphs][7] = Tw1_w2 of the last optimised keyframe (:899-910), d_stats5 [n_graphs][5] = iterations run, robust chi2
 * before / after, vertices, edges; h_ran[g] = 1 when graph g was optimised (0: no loop / a loop names an absent keyframe). */
int flvis_hip_pgo_loop_closure(flvis_ctx* ctx, int n_graphs, const int* h_n_kf, double* d_T_c_w7, const uint8_t* h_present,
                               const int* h_n_loops, const int* h_loop_ids, const double* d_loop_pose7, int iterations,
                               int use_initial_guess, double* d_drift7, double* d_stats5, int* h_ran);

/* ---- pipeline-level entry points: F2FTracking + LocalMap for a batch of independent streams ------------------------
 *
 * Mirrors the reference's class surface (include/f2f_tracking.h:51-73, src/backend/vo_localmap.cpp:87-380):
 *   flvis_config_load        <- TrackingNodeletClass::onInit yaml handling      src/frontend/vo_tracking.cpp:103-306
 *                                (accepts the reference's yaml files unchanged; src/utils/include/yamlRead.h)
 *   flvis_tracker_create     <- F2FTracking::init                               src/frontend/f2f_tracking.cpp:5-38
 *   flvis_imu_feed(_out)     <- TrackingNodeletClass::imu_callback + F2FTracking::imu_feed (_out: with its q_w_i / pos_w_i / vel_w_i)
 *   flvis_get_imu_states     <- the same outputs, batched
 *                                                                               src/frontend/vo_tracking.cpp:326-371, f2f_tracking.cpp:46-57
 *   flvis_image_feed         <- F2FTracking::image_feed (+ KeyFrameMsg::pub + LocalMapNodeletClass::frame_callback when
 *                                with_local_map != 0)                           f2f_tracking.cpp:59-400, vo_tracking.cpp:396-430
 *   flvis_get_keyframe       <- flvis/KeyFrame message payload                  msg/KeyFrame.msg, src/utils/keyframe_msg.cpp:30-124
 *   flvis_get_correction     <- flvis/CorrectionInf message payload             msg/CorrectionInf.msg, src/utils/correction_inf_msg.cpp:13-64
 *   flvis_ba_push_keyframe   <- LocalMapNodeletClass::frame_callback alone      src/backend/vo_localmap.cpp:87-380
 */
typedef struct flvis_cfg {
  int type_of_vi;                 /* 1 EuRoC (stereo unrectified + IMU), 3 D435i stereo, 5 D435 stereo + pixhawk,
                                     0 D435i depth, 2 D435 depth + pixhawk (the second image is the Z16 depth image),
                                     4 KITTI (rectified stereo, no IMU: the rig is given by cam{0,1}_projection_matrix, which
                                     flvis_config_load stores in P0 / P1 and flvis_config_finalize turns into K, T_cam0_cam1;
                                     src/frontend/vo_tracking.cpp:146,265-306) */
  int image_width, image_height;
  double cam0_intrinsics[4], cam0_distortion[4], cam1_intrinsics[4], cam1_distortion[4];
  double T_imu_cam0[16];          /* row-major 4x4 (EuRoC: T_imu_mavimu * T_mavimu_cam0) */
  double T_cam0_cam1[16];
  double vifusion_para[6], feature_para[6], dr_para[3];
  int window_size;
  /* derived by flvis_config_finalize (cv::stereoRectify restated, CALIB_ZERO_DISPARITY, alpha 0) */
  int cam_type, imu_type, skip_first_n_imgs, need_equal_hist;
  double R0[9], R1[9], P0[12], P1[12];
  double depth_factor;            /* depth modes: Z16 units per metre (yaml key depth_factor, vo_tracking.cpp:153) */
} flvis_cfg;

typedef struct flvis_frame_out {
  int state;            /* 0 UnInit, 1 Tracking, 2 TrackingFail (enum TRACKINGSTATE) */
  int new_keyframe, reset_cmd, n_landmarks;
  int64_t frame_id;
  double T_c_w[7];      /* tx ty tz qx qy qz qw of curr_frame */
  int of_inliers, f_inliers, pnp_inliers, pad_;   /* the counts lkorb_tracking.cpp:191 prints */
  double reprojection_error;
} flvis_frame_out;

int flvis_config_load(const char* yaml_path, flvis_cfg* cfg, char* err, int errlen);
int flvis_config_finalize(flvis_cfg* cfg);
/* One boolean key of the same yaml file, as getBoolVariableFromYaml reads it (yamlRead.h: yaml-cpp 0.6.2 as<bool>): the plain scalars
 * y / n, yes / no, true / false, on / off, each all lower case, Capitalised or all UPPER case.  *out = 1 or 0.  The keys the nodelets read
 * this way and flvis_cfg does not carry: output_sparse_map (vo_localmap.cpp: flvis_local_map_cloud is that output), is_lite_version.
 * FLVIS_ERR_CONFIG with a message in err: the file cannot be opened, the key is missing, the value is anything else (mixed case, a number,
 * nothing).  FLVIS_ERR_INVALID_ARG: a NULL path, key or out.  Host only. */
int flvis_config_get_bool(const char* yaml_path, const char* key, int* out, char* err, int errlen);

/* CameraFrame::recover3DPts_c_FromStereo (src/processing/camera_frame.cpp:93-180) in ONE call -- the kernel-level drop-in a
 * configs[1] integrator (the reference's own frame loop, HIP pieces underneath) puts in its place: the stereo matcher's seeds
 * (the pixel itself, or for landmarks with depth the world point projected into camera 1 with T_cam1_cam0 * T_c_w, :108-122),
 * cv::calcOpticalFlowPyrLK(img0, img1, 31 x 31, maxLevel 5, 30 iterations / 0.001, OPTFLOW_USE_INITIAL_FLOW, :124-128),
 * cv::undistortPoints(K1, D1, R1, P1) (:130-131), Triangulation::trignaulationPtFromStereo with the rig's P0 / P1 (valid unless
 * z < 0 or z > range) and, for every landmark whose match or triangulation failed, the rand()-drawn dummy depth 0.3 + rand() / (RAND_MAX
 * / 0.4) through its undistorted pixel (:149-176) -- drawn in landmark order, as the reference's loop calls rand().
 * A "set" is one frame (n_sets frames of independent streams are matched in one launch).  Per set s, landmark i < d_count[s] (arrays
 * [n_sets][cap]...): d_pt2d_plane / d_pt2d_undistort / d_pt3d_w / d_has_depth = what getAll2dPlaneUndistort3d_cvPf and hasDepthInf()
 * hand the reference (cv::Point2f / Point3f: float); h_T_c_w7 (host, [n_sets][7], tx ty tz qx qy qz qw) the frame's pose.
 * d_img0 / d_img1: device [n_sets][h][w] mono8 of cfg's image size.  range: the float the reference passes (dr_para2).
 * d_rand_state35: the glibc generator of each set, [n_sets][35] int32 on the device, in / out -- flvis_hip_rand_seed(seed) initialises it
 * like srand(seed) (seed 1: a process that never called srand, which is what the reference is); consecutive calls continue the sequence.
 * Outputs: d_pt3d_c [n_sets][cap][3] (pt3ds, camera frame) and d_mask_has_3d [n_sets][cap] (maskHas3DInf).
 * Returns FLVIS_ERR_CONFIG for a depth-camera rig (recover3DPts_c_FromDepthImg is the tracker's own, flvis_image_feed). */
int flvis_hip_rand_seed(flvis_ctx* ctx, uint32_t seed, int32_t* d_state35, int n_sets);
int flvis_hip_stereo_depth(flvis_ctx* ctx, const flvis_cfg* cfg, const uint8_t* d_img0, const uint8_t* d_img1, int n_sets,
                           const float* d_pt2d_plane, const float* d_pt2d_undistort, const float* d_pt3d_w, const uint8_t* d_has_depth,
                           const int* d_count, int cap, const double* h_T_c_w7, float range, int32_t* d_rand_state35, double* d_pt3d_c,
                           uint8_t* d_mask_has_3d);

/* LKORBTracking::tracking(from, to, T_c_w_guess, use_guess, ...) (src/processing/lkorb_tracking.cpp:9-202) in ONE call, for n_sets independent
 * frames (a set is one frame) and every cam_type of cfg: no host step between the optical flow and the pose.
 * In, per set s and landmark i < d_count[s] (arrays [n_sets][cap]...; a count above cap reads as cap, a negative one as 0): d_img_from /
 * d_img_to [n_sets][h][w] mono8 of cfg's image size (from.img0 / to.img0); d_from_2d_plane / d_from_2d_undistort / d_from_3d_w what
 * getAll2dPlaneUndistort3d_cvPf hands the reference (cv::Point2f / Point3f); d_from_flags bit 0 has_3d, bit 1 is_tracking_inlier of
 * from.landmarks[i] (the copy `lm = from.landmarks.at(i)` carries the flag over and the F step only ever clears it, so it is an input);
 * h_guess7 [n_sets][7] (tx ty tz qx qy qz qw) and h_use_guess [n_sets], host, per set and freely mixed; h_use_guess NULL: no set has a guess
 * (h_guess7 may then be NULL too).
 * Steps: the seeds -- from_2d_plane, or with a guess cv::projectPoints(K0, D0) on stereo rigs and, on CAM_DEPTH, camera2pixel of the
 * float-narrowed landmark (:41-58) --; cv::calcOpticalFlowPyrLK(31 x 31, maxLevel 10, 30 / 0.001, OPTFLOW_USE_INITIAL_FLOW, minEig 1e-4) with the
 * pyramids of flvis_hip_lk_track; on STEREO_UNRECT cv::undistortPoints(K0, D0, R0, P0) of the tracked points (the other rigs use the plane
 * coordinates on both sides, whatever d_from_2d_undistort holds); the survivors (status 1, 0 < x < w - 1, 0 < y < h - 1) into `to` in
 * DESCENDING index order; fewer than 10: ret 0.  cv::findFundamentalMat(FM_RANSAC, 5.0, 0.99) on the ascending pairs; mask[i] == 0 clears
 * is_tracking_inlier of to.landmarks[i] (the reference's mirrored index, kept); fewer than 10 flags left: ret 0, the pose untouched.  The pairs
 * has_3d && is_tracking_inlier in `to` order go to cv::solvePnPRansac(100, 3.0, 0.99) with the rectified K (P0) -- SOLVEPNP_ITERATIVE from the
 * guess, SOLVEPNP_P3P without --, CameraFrame::updateLMState clears the flag of the pairs outside its mask, ret = inliers >= 10.
 * Out: to.landmarks as d_to_from [n_sets][cap] (index in `from` of the j-th landmark of `to`), d_to_2d_plane / d_to_2d_undistort, d_to_flags;
 * d_mask_F [n_sets][cap] (may be NULL) the F mask by ascending survivor rank; d_counts4 [n_sets][4] = of_inlier_cnt, F_inlier_cnt, the pairs
 * handed to the PnP, pnp_inlier_cnt (0 for a stage not reached); d_pose7 [n_sets][7] in / out: written by the sets that reach the PnP (when it
 * finds no model: the guess as a rotation matrix turned into a quaternion again, or the identity), left alone by the others; d_ret [n_sets].
 * Rows of `to` from of_inlier_cnt on are never written.  A set's result is a function of that set alone; the host arrays may be freed when the
 * call returns.
 * Refused before anything is launched or written: null pointers, n_sets <= 0 or > 65535, cap <= 0, a non-zero h_use_guess entry with h_guess7
 * NULL (FLVIS_ERR_INVALID_ARG); cap > 1024 (FLVIS_ERR_CAPACITY: the F search and the PnP hold 1024 points; the call never truncates); an
 * image below 32 x 32 or a configuration that did not go through flvis_config_finalize (FLVIS_ERR_CONFIG).  One flvis_cfg per call. */
int flvis_hip_lkorb_tracking(flvis_ctx* ctx, const flvis_cfg* cfg, const uint8_t* d_img_from, const uint8_t* d_img_to, int n_sets,
                             const float* d_from_2d_plane, const float* d_from_2d_undistort, const float* d_from_3d_w,
                             const uint8_t* d_from_flags, const int* d_count, int cap, const double* h_guess7, const uint8_t* h_use_guess,
                             int* d_to_from, float* d_to_2d_plane, float* d_to_2d_undistort, uint8_t* d_to_flags, uint8_t* d_mask_F,
                             int* d_counts4, double* d_pose7, uint8_t* d_ret);

/* Creates the batched tracker (and local map) for n_streams independent streams inside `ctx`.  seed_base + stream is the
 * RANSAC seed of each stream.  traj_capacity > 0 keeps a device-side trajectory of that many frames per stream. */
int flvis_tracker_create(flvis_ctx* ctx, const flvis_cfg* cfg, int n_streams, uint64_t seed_base, int traj_capacity);
/* The same with one finalized config per stream (cfgs[0 .. n_streams)): a batch of cameras that are calibrated each on its own.
 * Stream s behaves bit for bit as stream s of flvis_tracker_create(ctx, &cfgs[s], n_streams, seed_base, traj_capacity).
 * Per stream: the intrinsics and distortion of both cameras, R0 / R1 / P0 / P1, T_imu_cam0, T_cam0_cam1, depth_factor, dr_para and
 * vifusion_para.  Batch-wide -- every config must match cfgs[0] exactly, as they size buffers and pick code paths: type_of_vi (and so
 * cam_type, imu_type), image_width, image_height, feature_para[0..5], window_size, skip_first_n_imgs, need_equal_hist.  A config that
 * differs in one of them returns FLVIS_ERR_CONFIG (flvis_last_error names the field and the stream) and creates nothing: a tracker the
 * context already holds is kept.  Every check of flvis_tracker_create applies to each config.  (The loop closer's counterpart:
 * flvis_loop_closer_create_rigs.) */
int flvis_tracker_create_rigs(flvis_ctx* ctx, const flvis_cfg* cfgs, int n_streams, uint64_t seed_base, int traj_capacity);
/* The config stream `stream` runs on: the one it was created or last reset with (flvis_reset_streams_rigs). */
int flvis_get_stream_cfg(flvis_ctx* ctx, int stream, flvis_cfg* out);

/* Number of lanes (sub-batches with their own HIP streams and device state) the tracker splits its streams into.  One by
 * default; the environment variable FLVIS_LANES (1..16) is a tuning knob (more lanes measured slower on MI355X, DESIGN.md
 * section 4).  The partition changes no result (streams are independent). */
int flvis_tracker_lanes(flvis_ctx* ctx);
/* Trackers with more than one lane (FLVIS_LANES): by default the context's stream waits for every lane at the end of a call, so
 * that the caller may overwrite the input images in stream order right away -- which also keeps the lanes in step.  A caller that
 * cycles through n + 1 input buffers (leaves a call's images untouched during the next n calls) says so here (0 <= n <= 7); the
 * lanes may then run up to n frames apart and the image kernels of one lane overlap the geometry chain of another. */
int flvis_set_input_hold(flvis_ctx* ctx, int n_frames);
/* Tuning aid: host milliseconds inside flvis_image_feed since flvis_tracker_create: [0] total, [1] of it blocked on the pinned
 * upload ring, [2] calls. */
int flvis_debug_host_times(flvis_ctx* ctx, double* h_out3);
/* ... and of flvis_image_feed_host since the tracker was created: [0] ms blocked on the previous call's uploads (the hold_buffers contract),
 * [1] ms issuing this call's uploads, [2] ms inside flvis_image_feed, [3] calls. */
int flvis_debug_host_feed_times(flvis_ctx* ctx, double* h_out4);
/* ... and the uploads themselves: enable = 1 brackets every call's uploads with two timing events on the copy stream, 0 stops that, -1
 * leaves the setting; h_out3 (may be NULL) = [0] ms of the bracketed uploads that have finished, [1] their bytes, [2] their number.
 * (What bench.py's with_h2d.upload_GBs is made of: bytes / the copies' own durations, not the host's view.) */
int flvis_debug_host_feed_timing(flvis_ctx* ctx, int enable, double* h_out3);

/* One IMU sample of stream `stream` in the SENSOR frame; remapped per type_of_vi like imu_callback does.  Samples are
 * staged on the host and consumed by the next flvis_image_feed (feed samples with t <= image time before the image). */
int flvis_imu_feed(flvis_ctx* ctx, int stream, double t, const double* acc3, const double* gyro3);
/* Same, n samples already in the FLVIS IMU frame: rows of 7 doubles (t, acc xyz, gyro xyz). */
int flvis_imu_feed_flvis_frame(flvis_ctx* ctx, int stream, int n, const double* samples7);

/* All streams at once: h_counts [n_streams], h_samples [n_streams][samples_per_stream][7] (FLVIS IMU frame). */
int flvis_imu_feed_all(flvis_ctx* ctx, const int* h_counts, const double* h_samples, int samples_per_stream);

/* The outputs of F2FTracking::imu_feed(time, acc, gyro, q_w_i&, pos_w_i&, vel_w_i&) (src/frontend/f2f_tracking.cpp:46-57): the
 * propagated IMU state after every sample -- what imu_callback publishes as /imu_pose, /imu_odom and /imu_path
 * (src/frontend/vo_tracking.cpp:362-369) and what the EuRoC launch file records as the estimated trajectory
 * (launch/flvis_euroc_mav.launch:88,103).  During the attitude initialisation the reference returns the identity attitude and
 * zero position / velocity (vi_motion.cpp:39-40; the sample that sets the first attitude returns it, :60); so do these.
 *   flvis_imu_feed_out     the call-for-call form: the sample is integrated now (one small upload + kernel + read-back) and its
 *                          state is returned: q_w_i (w, x, y, z), pos_w_i, vel_w_i.  For a nodelet that publishes at IMU rate.
 *   flvis_get_imu_states   the batched form for the deferred path (flvis_imu_feed stages, the next flvis_image_feed integrates):
 *                          the rows written since the previous call for that stream, oldest first, at most cap; a row is
 *                          (t, qw, qx, qy, qz, px, py, pz, vx, vy, vz).  Samples still staged are integrated first.  The device keeps
 *                          the last 512 rows per stream; *n_dropped (may be NULL) = older rows lost since the previous call.
 * Both forms run the same device code in the same order as the next frame head would, so the values are identical. */
int flvis_imu_feed_out(flvis_ctx* ctx, int stream, double t, const double* acc3, const double* gyro3, double* q_w_i_wxyz,
                       double* pos_w_i3, double* vel_w_i3);
int flvis_get_imu_states(flvis_ctx* ctx, int stream, int cap, double* h_rows11, int* n_out, int* n_dropped);

/* n_steps frames in one call -- the caller's loop `imu_callback ... ; image_input_callback` (vo_tracking.cpp:326-430) for frames whose
 * images are already in HBM: per step the IMU samples of all streams (h_imu_counts [n_streams], h_imu_samples
 * [n_streams][imu_samples_per_stream][7] in the FLVIS IMU frame; h_imu_counts NULL: none) and the stereo pair (device pointers as for
 * flvis_image_feed, h_times [n_streams]).  Equivalent to calling flvis_imu_feed_all + flvis_image_feed n_steps times; h_call_ms (may be
 * NULL) receives the host milliseconds each step spent enqueuing.  The images of step k must stay untouched as flvis_image_feed says.
 * One scheduling difference, none in the results: between two steps of a call the local-map launch for a step's keyframes is enqueued
 * inside the NEXT step (behind its PnP RANSAC) instead of behind the step itself, so that the ~0.3 ms in which two local-map launches
 * overlap do not fall on the temporal LK.  The last step of a call launches at its end. */
typedef struct flvis_step {
  const uint8_t* d_img0;
  const uint8_t* d_img1;
  const double* h_times;
  const int* h_imu_counts;
  const double* h_imu_samples;
  int imu_samples_per_stream;
} flvis_step;
int flvis_run_steps(flvis_ctx* ctx, int n_steps, const flvis_step* steps, int with_local_map, double* h_call_ms);

/* Optional per-stage timing of flvis_image_feed with HIP events on the context's stream (for bench.py's roofline).
 * flvis_prof_enable(max_steps) arms it for the next max_steps frames; flvis_prof_read sums the elapsed ms per stage. */
int flvis_prof_enable(flvis_ctx* ctx, int max_steps);
/* Same, but only the stages whose bit is set in stage_mask record events (an event record costs a few microseconds on
 * the GPU queue; timing all ~20 stages inflates a frame by ~10%). */
int flvis_prof_enable_stages(flvis_ctx* ctx, int max_steps, uint64_t stage_mask);
int flvis_prof_stage_count(void);
const char* flvis_prof_stage_name(int i);
int flvis_prof_read(flvis_ctx* ctx, double* h_ms_per_stage, int* n_steps);
/* Per-frame elapsed ms of one enabled stage (stage "frame(chain)" = the whole main-stream chain of a frame, i.e. the GPU
 * latency of one batch step); returns the number of frames written (<= cap). */
int flvis_prof_read_steps(flvis_ctx* ctx, int stage, double* h_ms, int cap);

/* One stereo frame for every stream of the batch.  d_img0/d_img1: device [n_streams][h][w] mono8; h_times: host
 * [n_streams] seconds.  h_out (host, [n_streams], may be NULL): results; when NULL nothing is copied back and the call
 * does not synchronise.  with_local_map != 0 also runs the sliding-window BA for streams that emit a keyframe.
 * Depth-camera rigs (type_of_vi 0 / 2): d_img1 is the Z16 depth image aligned to cam0, [n_streams][h][w] uint16
 * (F2FTracking::image_feed(time, img0, d_img, ...), src/frontend/vo_tracking.cpp:453, f2f_tracking.cpp:116-119). */
int flvis_image_feed(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times,
                     flvis_frame_out* h_out, int with_local_map);

/* The same frame step with the images handed over as HOST buffers, the way TrackingNodeletClass::image_input_callback hands
 * two cv::Mat to F2FTracking::image_feed (src/frontend/vo_tracking.cpp:396-430, f2f_tracking.cpp:59-119): one flvis_image
 * per stream and camera.  channels 1 (mono8), 3 (BGR) or 4 (BGRA) -- colour input is converted like cv::cvtColor does at
 * f2f_tracking.cpp:74-111; on depth rigs h_img1 is the 16UC1 depth image (channels 1, 2 bytes per pixel, pitch in bytes).
 * The stamp of a stream's frame is h_img0[stream].t.  Rows may be padded (pitch >= width * bytes per pixel).  The uploads
 * run asynchronously on a copy stream into double-buffered device staging, so the H2D transfer of a frame overlaps the
 * kernels of the previous one; page-locked host memory (hipHostMalloc / hipHostRegister) is what makes them truly async.
 * hold_buffers == 0: returns once the uploads are done (the caller may reuse its buffers immediately);
 * hold_buffers != 0: returns at once, the buffers must stay valid until the next call on this context returns. */
typedef struct flvis_image {
  const uint8_t* data;
  int width, height, pitch, channels;
  double t;
} flvis_image;
int flvis_image_feed_host(flvis_ctx* ctx, const flvis_image* h_img0, const flvis_image* h_img1, flvis_frame_out* h_out,
                          int with_local_map, int hold_buffers);

/* Per-stream frame presence: the frame step advances only the streams that have a new frame (cameras at different rates, dropped
 * frames, a camera that joins a running batch later).  h_present [n_streams]: nonzero = stream s has a frame in this step; NULL = every
 * stream has one, exactly the entry point without _present.  Stream s under any presence schedule returns bit for bit what stream s of
 * a tracker with the same configs, n_streams, seed_base and traj_capacity returns when it is fed only its present frames, each with the
 * IMU samples that arrived since its previous present frame: per-frame outputs, trajectory rows (row j = its j-th present frame),
 * landmarks, keyframe payloads, corrections, pose records, IMU-state rows and flvis_get_local_map_counts.  For a stream absent in a step:
 *   - its images are not read (device slots [s] may hold anything; host entry: h_img0[s] / h_img1[s] are not looked at, their data may
 *     be NULL, nothing of the stream is uploaded) and h_times[s] / h_img0[s].t is ignored;
 *   - the IMU samples staged for it are integrated in the step (imu_callback without an image): its IMU-state rows are those of the run
 *     fed its present frames alone;
 *   - nothing else of it changes: frame count, skip_first_n_imgs (counted in its own present frames), the rand() state, its image slots
 *     and template cache; no trajectory row, no keyframe.  Its h_out entry is its last frame's output (same frame_id: how a caller
 *     tells presence), all zero before its first frame since tracker creation or its last reset;
 *   - keyframes queued before keep being optimised.
 * A step in which no stream is present is legal (only the IMU advances).  flvis_get_counters [0] counts the frames of present streams.
 * A reset of an absent stream (flvis_reset_streams) takes effect in stream order: its next present frame is frame 0 of the new sequence.
 * Works with several lanes and flvis_set_input_hold, also for a lane in which no stream is present.
 * flvis_image_feed_host_present: a present stream with NULL data (or a size that does not match) returns FLVIS_ERR_INVALID_ARG before
 * anything is enqueued.  flvis_run_steps_present: h_present [n_steps][n_streams], row k for step k (NULL: all present). */
int flvis_image_feed_present(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times,
                             const uint8_t* h_present, flvis_frame_out* h_out, int with_local_map);
int flvis_image_feed_host_present(flvis_ctx* ctx, const flvis_image* h_img0, const flvis_image* h_img1, const uint8_t* h_present,
                                  flvis_frame_out* h_out, int with_local_map, int hold_buffers);
int flvis_run_steps_present(flvis_ctx* ctx, int n_steps, const flvis_step* steps, const uint8_t* h_present, int with_local_map,
                            double* h_call_ms);

/* Landmarks of curr_frame of one stream (host arrays of capacity cap): ids, raw pixel, rectified pixel, world point,
 * flags (bit0 has_3d, bit1 is_tracking_inlier).  Returns the landmark count (or <0). */
int flvis_get_landmarks(flvis_ctx* ctx, int stream, int cap, int64_t* h_id, double* h_2d, double* h_2d_undist,
                        double* h_3d_w, uint8_t* h_flags);
/* Last KeyFrame payload of a stream: returns lm_count (or <0); arrays of capacity cap. */
int flvis_get_keyframe(flvis_ctx* ctx, int stream, int cap, int64_t* frame_id, double* T_c_w7, int64_t* h_lm_id,
                       double* h_lm_2d, double* h_lm_3d);
/* The same keyframe as the full flvis/KeyFrame message (msg/KeyFrame.msg:1-11 as KeyFrameMsg::pub fills it,
 * src/utils/keyframe_msg.cpp:30-124): header.stamp, frame_id, command (KFMSG_CMD_NONE = 0; the reference's reset publisher is
 * commented out, vo_tracking.cpp:431 -- the reset request is flvis_frame_out.reset_cmd), the two images the tracker worked on
 * (img0: mono8 AFTER equalizeHist where the rig uses it; img1: mono8, or the 16UC1 depth image on depth rigs), lm_count with the
 * id / undistorted-pixel / world-point arrays, T_c_w; lm_descriptor_data is empty in the reference (:71-81).  The caller provides
 * the arrays (capacity cap) and, optionally, host buffers for the images (width * height bytes, 2 bytes per pixel for a depth
 * img1; NULL = not wanted).  Call it right after the flvis_image_feed that reported new_keyframe: the images are the
 * tracker's working copies of THAT frame.  LIFETIME: img0 is always the tracker's own copy; img1 is read through the pointer that
 * flvis_image_feed was given when the right / depth image is used in place (depth rigs, and stereo rigs without equalizeHist whose
 * rows are dword aligned): a caller of flvis_image_feed that wants img1 here must leave that device buffer untouched until this call
 * has returned (flvis_image_feed_host keeps its own double-buffered staging: nothing to observe there).
 * Returns lm_count (0: the stream's last frame was no keyframe; < 0: error). */
typedef struct flvis_keyframe {
  int64_t frame_id;
  int8_t command;
  double stamp;
  flvis_image img0, img1;       /* data = the host buffers passed in (or NULL), pitch = tightly packed */
  int32_t lm_count;
  const int64_t* lm_id;         /* the caller's arrays */
  const double* lm_2d;          /* [lm_count][2] undistorted pixel */
  const double* lm_3d;          /* [lm_count][3] world */
  double T_c_w[7];              /* tx ty tz qx qy qz qw */
} flvis_keyframe;
int flvis_get_keyframe_msg(flvis_ctx* ctx, int stream, int cap, flvis_keyframe* kf, int64_t* h_lm_id, double* h_lm_2d,
                           double* h_lm_3d, uint8_t* h_img0, uint8_t* h_img1);
/* Last CorrectionInf of a stream: returns 1 if one exists (0 if not yet, <0 error). */
int flvis_get_correction(flvis_ctx* ctx, int stream, int cap, int64_t* frame_id, double* T_c_w7, int* lm_count,
                         int64_t* h_lm_id, double* h_lm_3d, int* lm_outlier_count, int64_t* h_outlier_id);

/* Local-map feedback into the tracker.  F2FTracking::correction_feed (src/frontend/f2f_tracking.cpp:40-44):
 * the reference's v2 unpacks CorrectionInf in correction_feedback_callback (vo_tracking.cpp:373-385) and never calls it, so
 * this is opt-in -- a caller that never feeds a correction gets v2 behaviour.  The correction (e.g. what
 * flvis_get_correction returned) is applied at the stream's next Tracking frame exactly as f2f_tracking.cpp:189-219 does:
 * pose_records and last_frame->T_c_w are re-anchored on the corrected keyframe pose, lm_3d_w of the named landmarks is
 * overwritten, the named outliers lose is_tracking_inlier.  Host buffers; returns after the upload. */
int flvis_correction_feed(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T_c_w7, int lm_count,
                          const int64_t* h_lm_id, const double* h_lm_3d, int lm_outlier_count,
                          const int64_t* h_lm_outlier_id);
/* F2FTracking::pose_records (f2f_tracking.h:59) of a stream, oldest first: rows (frame_id, tx ty tz qx qy qz qw).
 * Returns the number of records (< 1000). */
int flvis_get_pose_records(flvis_ctx* ctx, int stream, int cap, double* h_rows8);
/* Device-side trajectory of one stream: rows of 9 doubles (t, tx ty tz qx qy qz qw, state | new_kf<<4). */
int flvis_get_trajectory(flvis_ctx* ctx, int stream, int first_frame, int n_frames, double* h_rows9);
/* Trajectory recorder (replaces src/independ_modules/vo_repub_rec.cpp:74-124 for offline runs): writes the recorded
 * camera poses T_w_c (inverse of T_c_w) of frames [first_frame, first_frame + n_frames) whose state is TRACKING to a
 * text file.  format 0: `stamp x y z qw qx qy qz` per line (vo_repub_rec.cpp:82-91, the TUM order with qw first);
 * format 1: KITTI, 12 row-major entries of [R | t] per line (:100-111).  min_dt > 0 emulates the recorder's throttle exactly
 * as written (:77-78): its `last_time` is set at the first call and never updated, so poses stamped within min_dt of the
 * first TRACKING pose are dropped and every later one is written (the reference: 0.1 s of wall clock).  Returns the number
 * of lines written or a negative error code. */
int flvis_write_trajectory(flvis_ctx* ctx, int stream, int first_frame, int n_frames, const char* path, int format,
                           double min_dt);
/* The recorder on /imu_pose (launch/flvis_euroc_mav.launch:83-103: vo_repub_rec, sub_type PoseStamped, sub_topic /imu_pose -> est.txt,
 * the trajectory the reference scores on EuRoC): writes rows of flvis_get_imu_states as `stamp x y z qw qx qy qz` (position pos_w_i,
 * attitude q_w_i; vo_repub_rec.cpp:74-91).  min_dt > 0: the throttle as written -- rows within min_dt of the FIRST row of the run are
 * dropped, every later one is written.  The run starts with the call that creates the file (append == 0): the throttle applies to that
 * call only; a batch that is appended (append != 0; flvis_get_imu_states hands out at most 512 rows per fetch) is written in full.
 * Returns the number of lines written, FLVIS_ERR_INVALID_ARG for bad arguments or FLVIS_ERR_CONFIG when the file cannot be opened. */
int flvis_write_imu_trajectory(const double* h_rows11, int n, const char* path, double min_dt, int append);
/* The same with the run's first stamp named by the caller (t_first = h_rows11[0] of the run's first batch; NaN: no throttle): rows
 * within min_dt of t_first are dropped in EVERY batch, also when the batch that created the file was shorter than min_dt
 * (the recorder's last_time is set once and never updated, vo_repub_rec.cpp:77-78). */
int flvis_write_imu_trajectory_run(const double* h_rows11, int n, const char* path, double min_dt, int append, double t_first);
/* Start over on the named streams (lane-independent indices in [0, n_streams)): from the next frame step on, each behaves exactly as
 * stream s of a tracker just made by flvis_tracker_create with the same cfg / seed_base / traj_capacity (F2FTracking::init + VIMOTION
 * ctor + an empty local map, src/frontend/f2f_tracking.cpp:5-38): frame ids, landmark ids (from 100), the dummy depth's rand() state,
 * skip_first_n_imgs, the IMU filter, the pose records, the trajectory rows (from row 0) and the local map all start over; time may go
 * backwards across the reset.  Discarded: IMU samples staged and not yet integrated, IMU-state rows not yet fetched, a correction
 * handed over with flvis_correction_feed and not yet applied, keyframes queued for the local map and not yet optimised (an optimisation
 * running at the reset publishes no correction that outlives it).  Other streams are not disturbed.  Duplicates are one reset; two
 * resets before the next frame step are one.  Enqueued in stream order; does not wait for the device.  n == 0: no-op.  A stream out of
 * range: FLVIS_ERR_INVALID_ARG and nothing changes.  The context-wide counters (flvis_get_counters(_n)) stay cumulative.  The
 * keyframe getters (flvis_get_keyframe, _msg, _imu, _imu_pos) return the stream's last keyframe since its last reset, none before the
 * next one.  The reset takes a keyframe-queue entry, which the tracker's back-pressure keeps free; should a full queue be met all the
 * same, the next flvis_hip_synchronize returns FLVIS_ERR_CAPACITY. */
int flvis_reset_streams(flvis_ctx* ctx, int n, const int* streams);
/* flvis_reset_streams with a new rig: stream streams[i] starts over on cfgs[i] (a duplicate: its last entry) and then equals stream
 * streams[i] of a tracker just made by flvis_tracker_create_rigs with that config in its place.  The reset's ordering holds for the rig
 * too: no frame or optimisation of the old sequence -- one already running, or a lane ahead under flvis_set_input_hold -- publishes
 * anything computed with the new rig, and nothing of the new sequence uses the old one.  Every config is checked first, as
 * flvis_tracker_create_rigs checks it against the tracker's batch-wide fields: one that fails returns FLVIS_ERR_CONFIG (or
 * FLVIS_ERR_CAPACITY) and nothing changes. */
int flvis_reset_streams_rigs(flvis_ctx* ctx, int n, const int* streams, const flvis_cfg* cfgs);
/* KFMSG_CMD_RESET_LM for the named streams' local maps alone (vo_localmap.cpp:87-98): keyframes queued before the command are
 * processed first, then the window, the graph and the keyframe deque are emptied and the optimiser returns to UN_INITIALIZED; the
 * published correction is withdrawn and the stream's flvis_get_local_map_counts entries start from 0.  The tracker is not touched.
 * The keyframe getters still return the stream's last keyframe.  Enqueued in stream order, in order with the keyframes; does not
 * wait for the device.  Arguments and errors as flvis_reset_streams. */
int flvis_local_map_reset(flvis_ctx* ctx, int n, const int* streams);
/* ---- the local map's sparse map cloud (/map_cloud, vo_localmap.cpp:329-377, :454-461; yaml key output_sparse_map) ----------------------
 * With output_sparse_map set the reference appends the optimised position of every multi-view landmark (bag->getMultiViewLMs(lms, 4)) to
 * `map` after each window optimisation and publishes the growing cloud.  Those are the lm_id / lm_3d of the CorrectionInf, which the next
 * optimisation overwrites (flvis_get_correction returns the last one).  The record keeps them on the device, per stream, without the host:
 * a small kernel behind every local-map launch (frame path, flvis_ba_push_keyframe*, the drains) appends the correction of a stream whose
 * window has optimised since the kernel last looked.  Opt-in: with the record off nothing is launched and nothing changes.
 * With the record on, every optimisation is looked at before the stream's next one overwrites it: a local-map launch then consists of
 * workers that take one keyframe per stream, each with the append kernel behind it (as many as the one worker would have taken
 * keyframes: FLVIS_BA_EVERY), and a lane's launches run one behind the other instead of overlapping on its two HIP streams.  That
 * order, not the kernel, is what the record costs: 6.8 % of the frame rate at 64 streams (profiles/r22_local_map_cloud.md).
 *
 * flvis_local_map_cloud_enable: after flvis_tracker_create(_rigs).  Room for max_points entries per stream (landmark id int64 + position
 *   3 doubles, the optimiser's own values: 32 bytes) and a header per stream.  max_points <= 0 switches the record off and frees it;
 *   enabling again, with the same capacity or another, starts empty.  Corrections from before the call are not recorded.  Waits for the
 *   device.  FLVIS_ERR_INVALID_ARG without a tracker, FLVIS_ERR_CAPACITY for max_points >= 2^31, FLVIS_ERR_HIP if the allocation fails
 *   (the record is then off).
 * A stream's record is at any time the concatenation of (lm_id[i], lm_3d[i]), i < lm_count, over a prefix of the stream's optimisations
 *   in order: what flvis_get_correction would have returned after each, in getMultiViewLMs order -- the reference's map->points.push_back
 *   order, duplicates across optimisations included.  An optimisation whose points do not fit whole is not recorded at all and counted as
 *   dropped; after the first dropped one nothing more is recorded until the stream is cleared (every later optimisation counts as
 *   dropped).  Capacity is the only cause.  (Should the kernel ever find that a window ran twice between two looks -- the launch
 *   order above excludes it -- it counts those runs as dropped too rather than leave a silent gap.)
 * flvis_local_map_reset (KFMSG_CMD_RESET_LM, which leaves `map` alone) leaves the record as it is, later optimisations append behind it.
 *   flvis_reset_streams(_rigs) empties the record of each named stream, and of no other, in order with the reset: nothing the old
 *   sequence's window still finishes is recorded.
 * flvis_local_map_cloud_clear: empties the named streams' records (points, runs, dropped).  Waits for the device.  Errors as
 *   flvis_reset_streams, and FLVIS_ERR_INVALID_ARG with the record off.
 * flvis_local_map_cloud_info: h_info4 = points recorded, optimisations recorded, optimisations dropped, capacity.  Waits for what is
 *   queued; does not drain the keyframe queues (flvis_get_local_map_counts does).
 *
 * flvis_local_map_cloud: the records of the n listed streams as n clouds.
 *   mode FLVIS_LM_CLOUD_ALL: every recorded entry, in record order -- the reference's cloud.  FLVIS_LM_CLOUD_LATEST: one entry per landmark
 *   id, the one from the newest recorded optimisation that lists the id, the survivors in record order (ids recur, and not in adjacent
 *   optimisations only: a landmark's view count falls below 4 and rises again).
 *   The selected entries of stream h_stream[c] are cloud c of flvis_hip_voxel_cloud: one row of fp64 points in canonical (record) order
 *   under an identity pose.  leaf, min_points, out_cap, d_xyz [n][out_cap][3], d_npts [n][out_cap] (may be NULL), h_n_out [n] (full
 *   counts; the first out_cap rows are written), h_n_dropped [n] (may be NULL: points that are not finite or outside the voxel range) and
 *   the rounding to float are that call's, bit for bit.  leaf == 0 is the reference's raw output: every point, rounded once to float.
 *   d_id [n][out_cap] (may be NULL; leaf == 0 only): the landmark id of each row.
 *   Several streams in one call give, stream for stream, the bits of single calls; a second call gives the same bits.  A stream with an
 *   empty record gives h_n_out = 0.  The call waits for its own counts (the _host form: and for its rows) and for nothing else; the
 *   tracker's and the local map's queued work is ordered ahead of it on the device.  No effect a caller can observe on tracking,
 *   corrections or the record.
 *   _host: h_xyz / h_npts / h_id are host arrays of the same shapes; the rows below min(h_n_out, out_cap) are written.
 *   FLVIS_ERR_INVALID_ARG before anything is queued: no tracker or the record is off; n <= 0; a NULL h_stream or h_n_out; a stream out of
 *   range or listed twice; an unknown mode; d_id with leaf > 0; leaf < 0 or not finite, min_points < 1, out_cap < 0, NULL rows with
 *   out_cap > 0.  FLVIS_ERR_CAPACITY: the listed records hold 2^31 entries or more together. */
#define FLVIS_LM_CLOUD_ALL    0
#define FLVIS_LM_CLOUD_LATEST 1
int flvis_local_map_cloud_enable(flvis_ctx* ctx, int64_t max_points);
int flvis_local_map_cloud_clear(flvis_ctx* ctx, int n, const int* streams);
int flvis_local_map_cloud_info(flvis_ctx* ctx, int stream, int64_t* h_info4);
int flvis_local_map_cloud(flvis_ctx* ctx, int n, const int* h_stream, int mode, double leaf, int min_points, int out_cap, float* d_xyz,
                          int* d_npts, int64_t* d_id, int64_t* h_n_out, int64_t* h_n_dropped);
int flvis_local_map_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, int mode, double leaf, int min_points, int out_cap, float* h_xyz,
                               int* h_npts, int64_t* h_id, int64_t* h_n_out, int64_t* h_n_dropped);
/* ---- the keyframe log (/vo_kf, KeyFrameMsg::pub, src/utils/keyframe_msg.cpp:30-124) ------------------------------------------------------
 * flvis_get_keyframe_msg returns a stream's LAST keyframe, and its images only until the next frame overwrites them: a keyframe born
 * inside a flvis_run_steps batch that is not its stream's last is gone when the call returns.  The log keeps, per stream and on the
 * device, the whole flvis/KeyFrame message of a prefix of the stream's keyframes in order, each as flvis_get_keyframe_msg would have
 * returned it right after its frame: img0 (the tracker's level 0, AFTER equalizeHist where the rig uses it, rows tightly packed), img1
 * (mono8, or the Z16 depth image on depth rigs, tightly packed) and the payload (frame_id, stamp, T_c_w, lm_count, ids, undistorted
 * pixels, world points).  Opt-in: with the log off no kernel is launched and nothing changes.
 * With the log on, every lane's frame step launches one k_kf_log_append on the lane's tracking stream directly behind k_frame_end; the
 * workgroups of a stream that made no keyframe in the step (absent under *_present included) retire at once.  No HIP stream is added.
 * The kernel is what the log costs: 13 us on the frame chain, 1.5 % of the frame rate at 64 streams (profiles/r23_keyframe_log.md).
 * Where the right / depth image is read in place from the caller's buffer (depth rigs; stereo rigs without equalizeHist whose rows are
 * whole 16-byte lanes at 16-byte aligned bases), the copy reads that buffer inside the frame step: the rule on the caller's buffers
 * that holds for the step (in stream order; flvis_set_input_hold) covers it.  Once copied the log owns the image: the LIFETIME clause
 * of flvis_get_keyframe_msg does not apply to flvis_keyframe_log_get.
 *
 * flvis_keyframe_log_enable: after flvis_tracker_create(_rigs).  Room for max_keyframes messages per stream: n_streams * max_keyframes *
 *   (width * height * (1 + bytes per pixel of img1) + 48 KB of payload) bytes.  max_keyframes <= 0 switches the log off and frees it;
 *   enabling again, with the same capacity or another, starts empty.  Keyframes from before the call are not logged.  Waits for the
 *   device.  FLVIS_ERR_INVALID_ARG without a tracker, FLVIS_ERR_CAPACITY if the size does not fit the index arithmetic, FLVIS_ERR_HIP if
 *   the allocation fails (the log is then off).
 * A keyframe that does not fit is not recorded and counted as dropped; after the first dropped one nothing more is recorded for the
 *   stream until it is cleared (every later keyframe counts as dropped): the record stays a prefix, and capacity is the only cause of a
 *   drop.  Nothing is ever written past a stream's record.
 * flvis_reset_streams(_rigs) empties the record of each named stream, and of no other, in order with the reset; flvis_local_map_reset
 *   leaves it alone.  Frames fed with with_local_map = 0 are logged as well.  Works with several lanes and flvis_set_input_hold.
 * flvis_keyframe_log_clear: empties the named streams' records (entries and dropped count).  Waits for the device.  Errors as
 *   flvis_local_map_cloud_clear: FLVIS_ERR_INVALID_ARG for a stream out of range, a bad list, and with the log off.
 * flvis_keyframe_log_info: h_info3 = keyframes logged, keyframes dropped, capacity.  Waits for what is queued.
 * flvis_keyframe_log_get: logged keyframe `index` (0 = the oldest) of the stream, arguments and result as flvis_get_keyframe_msg: returns
 *   lm_count (>= 0), or FLVIS_ERR_INVALID_ARG for an index that is not logged.  Waits for what is queued.
 * flvis_keyframe_log_images: device pointers to the entry's two images (tight rows; either may be NULL), valid until the stream is
 *   cleared or reset, the log is enabled again or switched off, or the tracker is destroyed.
 * info / get / images / clear with the log off: FLVIS_ERR_INVALID_ARG. */
int flvis_keyframe_log_enable(flvis_ctx* ctx, int max_keyframes);
int flvis_keyframe_log_clear(flvis_ctx* ctx, int n, const int* streams);
int flvis_keyframe_log_info(flvis_ctx* ctx, int stream, int64_t* h_info3);
int flvis_keyframe_log_get(flvis_ctx* ctx, int stream, int index, int cap, flvis_keyframe* kf, int64_t* h_lm_id, double* h_lm_2d,
                           double* h_lm_3d, uint8_t* h_img0, uint8_t* h_img1);
int flvis_keyframe_log_images(flvis_ctx* ctx, int stream, int index, const uint8_t** d_img0, const void** d_img1);
/* Counters: [0] frames fed, [1] keyframes, [2] BA runs.  Cumulative over the context's work: a stream reset does not take them back. */
int flvis_get_counters(flvis_ctx* ctx, int64_t* h_counters3);
/* The first n (1 .. 4) of: [0] frames fed, [1] keyframes, [2] BA runs, [3] keyframes dropped at a full keyframe queue -- what the
 * reference's /vo_kf subscriber (queue size 10, src/backend/vo_localmap.cpp:452-456) does when the local map is slower than the tracker.
 * The tracker's stream-ordered back-pressure keeps a queue below its capacity, so [3] stays 0 unless a caller pushes keyframes itself
 * (flvis_ba_push_keyframe) faster than it lets the local map run. */
int flvis_get_counters_n(flvis_ctx* ctx, int n, int64_t* h_counters);
/* Per stream (arrays of n_streams, either may be NULL): keyframes the tracker has emitted and optimisations the stream's local map has
 * run (one per keyframe once the window holds window_size keyframes, vo_localmap.cpp:211-214,292-366), both since the stream's last
 * reset (flvis_reset_streams, flvis_local_map_reset).  Drains the queues first. */
int flvis_get_local_map_counts(flvis_ctx* ctx, int64_t* h_keyframes, int64_t* h_ba_runs);
/* Test aid: poses (tx ty tz qx qy qz qw) of a stream's last Tracking frame right after PnP-RANSAC and after the pose-only LM
 * (the two fp64 stages of LKORBTracking::tracking / OptimizeInFrame::optimize), h_out21 = 3 x 7 doubles (the third: the pose the LM starts from). */
int flvis_debug_stage_poses(flvis_ctx* ctx, int stream, double* h_out21);
/* Test aid: the visual-inertial filter of a stream (VIMOTION, src/processing/vi_motion.cpp).  Synchronises and integrates the samples
 * staged since the last frame (as flvis_get_imu_states does), then returns the number of states in the filter's queue (at most
 * STATES_QUEUE_SIZE - 1 = 399) and writes the first `cap` of them, oldest first, as rows (t, qw qx qy qz, pos_w_i, vel_w_i) into
 * h_rows11; h_biases6 (may be NULL): acc_bias, gyro_bias; h_flags4 (may be NULL): has_imu, is_first_data, imu_initialized and the count. */
int flvis_debug_vi_state(flvis_ctx* ctx, int stream, int cap, double* h_rows11, double* h_biases6, int* h_flags4);
/* Measurement aid (bench.py's LK instruction budget): enable != 0 makes the tracker's two LK launches per frame count their Gauss-Newton
 * iterations and the points that iterated, per pyramid level, into flvis_debug_counters: [36 + 2 l], [37 + 2 l] temporal LK at level l,
 * [48 + 2 l], [49 + 2 l] stereo LK; and, over both launches, [61] templates the temporal LK took from the template cache (written by
 * the previous frame's stereo LK), [62] template patches and [63] search regions staged by the slow (index-reflecting) path, i.e.
 * blocks that leave the pyramids' physical border. */
int flvis_debug_lk_stats(flvis_ctx* ctx, int enable);
/* Test aid: the tracker's pyramid construction on its own (the kernels F2FTracking's frames go through: the walking kernels of
 * pyr_walk.hip where the image geometry allows, else the LDS-tile kernels, then k_pyr_border for what is left).  Builds levels 1 .. levels
 * of n_img images (w x h, tightly packed) with a physical BORDER_REFLECT_101 border of bx columns / by rows around every level, as
 * cv::buildOpticalFlowPyramid keeps it.  d_out: level l = 0 .. levels at consecutive offsets (each level block rounded up to 64 bytes),
 * a block being [n_img][h_l + 2 by][pitch_l] bytes with pitch_l = ((w_l + 15) & ~15) + 2 bx and pixel (0, 0) at row by, column bx.
 * ingest != 0: level 0 of d_out is the copy of the source (with border); 0: level 0 is read in place and its block is left untouched. */
int flvis_debug_pyramid(flvis_ctx* ctx, const uint8_t* d_src, int w, int h, int n_img, int levels, int bx, int by, int ingest, uint8_t* d_out,
                        size_t out_bytes);
/* Test aid: the corner-response pass of flvis_hip_gftt alone (cornerMinEigenVal + the 3x3 local maxima), with the kernel variant chosen
 * (0: LDS tiles, 1: strip-mined tiles, 2: wave walk with `rows` rows per chunk): per image the ordered bits of the maximum response, the
 * number of local maxima and their sort keys ~((ordered(response) << 32) | pixel offset), unsorted, in h_keys [n_img][key_cap]. */
int flvis_hip_debug_corner_response(flvis_ctx* ctx, const uint8_t* d_img, int w, int h, int n_img, int variant, int rows,
                                    uint32_t* h_max_bits, int* h_nkeys, uint64_t* h_keys, int key_cap);
/* Test aid: the corner-response kernel's square root against the correctly rounded sqrtf on every float whose bit pattern lies in
 * [first_bits, first_bits + n); *h_mismatches = arguments on which the two differ (0 over the kernel's domain, see eig_walk.hip). */
int flvis_hip_debug_sqrt_check(flvis_ctx* ctx, uint32_t first_bits, uint32_t n, uint64_t* h_mismatches);
/* Raw device counter block (64 x int64): [0..7] as above, [8..] per-phase cycle counters of the BA kernel, filled only by
 * builds with -DFLVIS_BA_PROF (tuning aid, not part of the reference interface).  In other builds the local-map solver's path:
 * [24] optimize() calls (two per optimisation: before and after the cull) whose records streamed through the LDS in chunks instead of
 * staying resident, [25] the largest chunk count of any call (a maximum over the lanes, not a sum); [28] optimisations whose last call
 * streamed, [29] their duration in 10 ns ticks. */
int flvis_debug_counters(flvis_ctx* ctx, int64_t* h_counters64);

/* LocalMapNodeletClass::frame_callback for one stream with a caller-supplied KeyFrame (host arrays).  Returns 1 and fills
 * the outputs when an optimisation ran, 0 while the window is still filling -- or once the window has exceeded BA_LMAX (4096
 * landmarks) or BA_EMAX (8192 observations): that stream's local map then stops until it is reset, and the next flvis_hip_synchronize
 * returns FLVIS_ERR_CAPACITY naming the stream and the limit. */
int flvis_ba_push_keyframe(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T_c_w7, int lm_count,
                           const int64_t* h_lm_id, const double* h_lm_2d, const double* h_lm_3d, int cap,
                           int64_t* out_frame_id, double* out_T_c_w7, int* out_lm_count, int64_t* out_lm_id,
                           double* out_lm_3d, int* out_outlier_count, int64_t* out_outlier_id);

/* ---- IMU rotation factor of the window BA (an ADDITION -- the reference's local map, src/backend/vo_localmap.cpp,
 * optimises reprojection edges only, so nothing here has a reference counterpart and everything is off by default).
 *
 * The tracker integrates the bias-corrected gyro samples between keyframes (the samples VIMOTION::viIMUPropagation consumes,
 * src/processing/vi_motion.cpp:78-100) into dq = R_body(previous keyframe)^T R_body(this keyframe); the preintegration travels with
 * the KeyFrame payload.  With the factor enabled, the window BA adds for every pair of consecutive keyframes the edge
 *     r = Log(dq^T R_b(a)^T R_b(b)),   R_b = R_c_w^T R_c_i,   information I3 / (sigma_gyro^2 dt)
 * next to the reprojection edges (pose-pose blocks in the reduced camera system).
 *   flvis_set_imu_factor       enable != 0 switches the edges on for every stream; sigma_gyro = gyro noise density [rad/s/sqrt(Hz)]
 *   flvis_get_keyframe_imu     the preintegration of the stream's last keyframe: dq (w, x, y, z), dt [s]; returns 1 when it links
 *                              the keyframe to its predecessor, 0 otherwise (first keyframe after an initialisation, no IMU)
 *   flvis_ba_push_keyframe_imu flvis_ba_push_keyframe with the preintegration of the pushed keyframe (imu_dt <= 0: none) */
int flvis_set_imu_factor(flvis_ctx* ctx, int enable, double sigma_gyro);
/* The factor's position rows (an addition as the rotation rows are; off by default): between consecutive keyframes a -> b
 *   r_p = R_b(a)^T (p_b(b) - p_b(a) - v_a dt + 1/2 g_w dt^2) - dp,      information I3 / (sigma_acc^2 dt^3 / 3),
 * with dp = sum (dv dt + 1/2 dR f dt^2), dv = sum dR f dt the position / velocity preintegration of the bias-corrected accelerometer
 * samples (VIMOTION's convention: world acceleration = R f - g_w, g_w = (0, 0, -9.81)), and v_a the tracker's filter velocity at keyframe a,
 * a fixed quantity: there is no velocity or bias vertex, the pose blocks stay 6-dimensional.
 *   flvis_set_imu_factor_accel     sigma_acc > 0 [m/s^2/sqrt(Hz)] adds the rows to every IMU edge (flvis_set_imu_factor must be on); <= 0: off
 *   flvis_get_keyframe_imu_pos     dp (body frame of the previous keyframe) and v_a (world frame) of the stream's last keyframe; returns 1
 *   flvis_ba_push_keyframe_imu_pos flvis_ba_push_keyframe_imu with dp / v_a of the pushed keyframe */
int flvis_set_imu_factor_accel(flvis_ctx* ctx, double sigma_acc);
int flvis_get_keyframe_imu_pos(flvis_ctx* ctx, int stream, double* dp3, double* va3);
int flvis_ba_push_keyframe_imu_pos(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T_c_w7, const double* imu_dq_wxyz,
                                   double imu_dt, const double* imu_dp3, const double* imu_va3, int lm_count, const int64_t* h_lm_id,
                                   const double* h_lm_2d, const double* h_lm_3d, int out_cap, int64_t* out_frame_id, double* out_T_c_w7,
                                   int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d, int* out_outlier_count,
                                   int64_t* out_outlier_id);
int flvis_get_keyframe_imu(flvis_ctx* ctx, int stream, double* dq_wxyz, double* dt);
int flvis_ba_push_keyframe_imu(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T_c_w7, const double* imu_dq_wxyz,
                               double imu_dt, int lm_count, const int64_t* h_lm_id, const double* h_lm_2d, const double* h_lm_3d,
                               int cap, int64_t* out_frame_id, double* out_T_c_w7, int* out_lm_count, int64_t* out_lm_id,
                               double* out_lm_3d, int* out_outlier_count, int64_t* out_outlier_id);

/* ---- the loop-closing nodelet's control flow for a batch of independent sequences --------------------------------
 * LoopClosingNodeletClass (src/backend/vo_loopclosing.cpp:118-1119) without ROS: the keyframe database stays on the device.
 *   flvis_lc_params_load             <- onInit's LC_PARAS block                  :955-963
 *   flvis_loop_closer_create(_rigs)  <- onInit (camera from the same yaml, vocabulary already in the context: :1095-1101)
 *   flvis_loop_closer_add_keyframes  <- frame_callback + kfmsgProcess            :178-391
 *   flvis_loop_closer_process        <- one pass of pgoProcess per new keyframe  :393-518 (+ :520-944)
 * The reference's pgoProcess thread polls the newest keyframe (a keyframe may be examined twice or never); here every keyframe is
 * examined exactly once, in order. */
typedef struct flvis_lc_params {
  int lcKFStart, lcKFDist, lcKFMaxDist, lcKFLast, lcNKFClosest, minPts; /* lcKFStart / lcKFLast are read but unused by the reference too */
  double ratioMax, ratioRansac, minScore;
} flvis_lc_params;
typedef struct flvis_lc_event {
  int64_t kf_prev, kf_curr;  /* kf_curr = -1: the sequence had no new keyframe; kf_prev = -1: no candidate */
  int candidate;             /* isLoopCandidate */
  int n_matches, n_inliers;  /* mutual + ratio matches (p3d.size()), inliers of solvePnPRansac */
  int loop_accepted;         /* isLoopClosureKF: the loop went into loop_ids / loop_poses */
  int optimised;             /* loopClosureOnCovGraphG2ONew ran (:492-497) */
  int pgo_iterations;
  double loop_pose7[7];      /* se_ji (tx ty tz qx qy qz qw): the later keyframe's camera from the earlier one's */
  double chi2_before, chi2_after;
} flvis_lc_event;
typedef struct flvis_loop_closer flvis_loop_closer;
int flvis_lc_params_load(const char* yaml_path, flvis_lc_params* prm, char* err, int errlen);
/* cfg: flvis_config_load of the same yaml (image size, cam_type, rectified P0 / P1); the vocabulary must be resident
 * (flvis_hip_bow_load_vocabulary).  max_keyframes slots per sequence are allocated up front (76 KB each).  h_orb_pattern: see
 * flvis_hip_orb_detect_and_compute (NULL = the built-in pattern). */
int flvis_loop_closer_create(flvis_ctx* ctx, const flvis_cfg* cfg, const flvis_lc_params* prm, int n_streams, int max_keyframes,
                             const int8_t* h_orb_pattern, flvis_loop_closer** out);
/* The same with one finalized config per sequence (cfgs[0 .. n_streams)): a fleet of cameras that are calibrated each on its own, closed in
 * one batch.  Sequence s behaves bit for bit as sequence s of flvis_loop_closer_create(ctx, &cfgs[s], ...); flvis_loop_closer_create is this
 * call on n_streams copies of cfg.  Per sequence: what the closer reads from a config for geometry -- P0 and P1 (the stereo triangulation),
 * and with them K = P0[0], P0[5], P0[2], P0[6] (the depth camera's back-projection and the solvePnPRansac of the geometric check).
 * Batch-wide -- every config must match cfgs[0]: cam_type, image_width, image_height (they size buffers and pick the kernels' paths); so are
 * prm and the ORB pattern.  A config that differs in one of them returns FLVIS_ERR_CONFIG (flvis_last_error names the field and the
 * sequence) and creates nothing.  No other field is read.  depth_factor in particular is neither checked nor used: the depth camera's
 * branch divides the Z16 value by 1000, an integer division, as the reference writes it (vo_loopclosing.cpp:331), whatever the yaml says. */
int flvis_loop_closer_create_rigs(flvis_ctx* ctx, const flvis_cfg* cfgs, const flvis_lc_params* prm, int n_streams, int max_keyframes,
                                  const int8_t* h_orb_pattern, flvis_loop_closer** out);
/* Start over on the named sequences (distinct indices in [0, n_streams)): from the next call on, each returns bit for bit what sequence 0
 * of a closer just created on that sequence's config returns for the same keyframes -- keyframe ids from 0, events, similarity rows,
 * flvis_loop_closer_keyframe contents, poses and drift.  Emptied: the keyframes (the slot's whole max_keyframes capacity is free again),
 * T_odom_map (the identity), the loop list, the pose graph's trigger, the newest similarity row; a keyframe that was added and not yet
 * processed is discarded (the next flvis_loop_closer_process reports kf_curr = -1 for the sequence).  Until the sequence's next keyframe
 * flvis_loop_closer_poses and _similarity_row give *n_out = 0 and flvis_loop_closer_keyframe fails for every index.  The other sequences are
 * not disturbed.  n == 0: no-op.  A stream out of range or listed twice: FLVIS_ERR_INVALID_ARG and nothing changes.  Returns without
 * waiting for the device.
 * _rigs: sequence streams[i] also changes to the camera of cfgs[i] (another unit taking over the slot; the table on the device is updated
 * in stream order from memory the closer owns: cfgs may go away on return).  Every config is checked first against the closer's batch-wide
 * fields as flvis_loop_closer_create_rigs checks it: one that differs returns FLVIS_ERR_CONFIG and nothing changes.  A tracker slot and
 * its closer slot change hands together: flvis_reset_streams_rigs + flvis_loop_closer_reset_rigs. */
int flvis_loop_closer_reset(flvis_loop_closer* lc, int n, const int* streams);
int flvis_loop_closer_reset_rigs(flvis_loop_closer* lc, int n, const int* streams, const flvis_cfg* cfgs);
/* The config sequence `stream` runs on: the one it was created or last reset with. */
int flvis_loop_closer_stream_cfg(flvis_loop_closer* lc, int stream, flvis_cfg* out);
/* Loop closing on a STEREO_UNRECT rig (cam_type 1, the EuRoC camera).  By default (0) such a closer is the reference's: its case is empty,
 * a keyframe stores no landmark, and process / localize / link never verify a pair.  enable != 0 makes every frame that goes through a
 * keyframe's steps -- add_keyframes(_host) and the queries of localize(_host) and localize_in(_host) -- use the rule of
 * flvis_hip_lc_keyframe_landmarks_unrect with the rig of the frame's sequence (the configs of create_rigs / reset_rigs, which
 * flvis_loop_closer_stream_cfg returns: K, D of both cameras, R0, R1, P0, P1 per sequence).  An addition of this project, hence opt-in.
 * On such a closer flvis_loop_closer_keyframe returns pixels of the RECTIFIED plane, and every pose (loop_pose7, cand_pose7, T_c_map7,
 * flvis_loop_closer_poses; and so the T_c_w_odom7 a caller hands in) is of the RECTIFIED camera-0 frame -- the tracker's T_c_w on this rig.
 * The switch belongs to the whole database: FLVIS_ERR_INVALID_ARG while any sequence holds a keyframe (allowed again once every sequence
 * has been reset) and for a NULL closer; FLVIS_ERR_CONFIG on a closer whose cam_type is not 1.  Closers of cam_type 0 and 2 are untouched. */
int flvis_loop_closer_set_stereo_unrect(flvis_loop_closer* lc, int enable);
/* (destroy it before the context it was created on: every other call runs on that context's stream) */
void flvis_loop_closer_destroy(flvis_loop_closer* lc);
/* one keyframe for each of the n sequences h_stream[i] (distinct): d_img0 [n][h][w] mono8, d_img1 [n][h][w] mono8 (stereo) or Z16
 * (depth camera), h_T_c_w_odom7 [n][7] the tracker's pose of the keyframe (KeyFrame.msg T_c_w).  h_kf_id (optional): the keyframe's
 * index in its sequence. */
int flvis_loop_closer_add_keyframes(flvis_loop_closer* lc, int n, const int* h_stream, const uint8_t* d_img0, const void* d_img1,
                                    const double* h_T_c_w_odom7, int64_t* h_kf_id);
/* the same on HOST images (what KeyFrameMsg::unpack hands the nodelet, :206): h_img0[i] mono8, h_img1[i] mono8 or 16UC1, pitch in bytes */
int flvis_loop_closer_add_keyframes_host(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0,
                                         const flvis_image* h_img1, const double* h_T_c_w_odom7, int64_t* h_kf_id);
/* examines the newest keyframe of every sequence that got one since the last call; h_events [n_streams] */
int flvis_loop_closer_process(flvis_loop_closer* lc, flvis_lc_event* h_events);
/* The tracker's keyframe log (flvis_keyframe_log_enable) into the closer: every logged keyframe of every stream, no image leaving the
 * device.  The closer's context must be the one that holds the tracker, and the tracker's n_streams, image_width, image_height and
 * cam_type must be the closer's (FLVIS_ERR_CONFIG); with no tracker or the log off, FLVIS_ERR_INVALID_ARG.  Waits for the tracker's
 * queued work, reads the streams' counts in one copy, and works in rounds r = 0 .. max logged - 1: the streams that have an r-th entry
 * are round r's batch, in stream order; their images are gathered into one contiguous batch on the device and the round is exactly
 * flvis_loop_closer_add_keyframes with the logged T_c_w as T_c_w_odom -- followed, with process != 0, by flvis_loop_closer_process,
 * whose events are row r of h_events [events_cap][n_streams] (may be NULL).  *n_rounds (may be NULL): the number of rounds.
 * EQUIVALENCE: sequences are independent in the closer and a stream has at most one keyframe per frame step, so every sequence ends up
 * bit for bit as if add_keyframes / process had been called after each of its keyframes: database, similarity rows, events, poses, drift.
 * All or nothing, checked before anything is stored: a sequence whose keyframes + logged entries exceed max_keyframes:
 * FLVIS_ERR_CAPACITY; process with h_events and events_cap < rounds: FLVIS_ERR_INVALID_ARG.  A stream whose log dropped keyframes is NOT
 * refused: the closer gets the logged prefix, and flvis_keyframe_log_info tells the caller.  The log is not consumed: feeding twice
 * stores twice (flvis_keyframe_log_clear between batches).  flvis_loop_closer_set_stereo_unrect is honoured as by add_keyframes. */
int flvis_loop_closer_add_logged(flvis_loop_closer* lc, int process, flvis_lc_event* h_events, int events_cap, int* n_rounds);
/* kf_map_lc[i]->T_c_w of one sequence (host, [cap][7]); *n_out = keyframes in the sequence */
int flvis_loop_closer_poses(flvis_loop_closer* lc, int stream, double* h_T_c_w7, int cap, int* n_out);
/* one keyframe of the device-resident database on the host (KeyFrameLC, :100-112): the kept ORB landmarks (pixel, camera-frame position,
 * descriptor; arrays of capacity cap) and the bag-of-words vector; any output pointer may be NULL; the counts are the full counts */
int flvis_loop_closer_keyframe(flvis_loop_closer* lc, int stream, int kf, int cap, float* h_lm_2d, double* h_lm_3d, uint8_t* h_lm_desc,
                               int* lm_count, int* h_bow_ids, double* h_bow_vals, int* bow_count);
/* T_odom_map (:138, the tf map -> odom the nodelet broadcasts is its inverse) */
int flvis_loop_closer_drift(flvis_loop_closer* lc, int stream, double* h_T_odom_map7);
/* the newest row of the sequence's similarity matrix as the last flvis_loop_closer_process computed it */
int flvis_loop_closer_similarity_row(flvis_loop_closer* lc, int stream, double* h_row, int cap, int* n_out);
/* Relocalisation: where is a frame's camera in the map its sequence has built?  (The reference has no such call: a tracker that lost its
 * pose restarts at the identity and nothing ties the new odometry frame to the old map.  What follows is the reference's own pair check,
 * isLoopClosureKF :593-686, applied to (database keyframe, query) around a candidate choice that is this project's definition.)
 * Query: one image pair for each of the n sequences h_stream[i] (distinct), in the layout and types of flvis_loop_closer_add_keyframes.  It
 * goes through a keyframe's steps -- ORB, the bag of words of all descriptors, the landmarks with the sequence's own camera, the kept lists
 * -- and is NOT stored.  Database: everything add_keyframes has stored for the sequence, processed or not; an empty sequence gives
 * n_candidates = 0 and best = -1, not an error.
 * Candidates: the n_best (1 .. FLVIS_LC_FIX_CAND) keyframes with the highest L1 score against the query (flvis_hip_bow_score's value, bit
 * for bit) among those with score > 0 and score >= prm.minScore, by score descending and, for equal scores, keyframe index ascending;
 * n_candidates may be smaller than n_best.  No temporal exclusion (lcKFDist / lcKFMaxDist) and no 50-keyframe gate.
 * Pair check per candidate, exactly as flvis_loop_closer_process does it: mutual / ratio matches with prm.ratioMax; the keyframe's 3-D
 * point with the query's pixel; solvePnPRansac in its P3P form (100 iterations, 2.0 px, 0.99) with the sequence's K; cand_accepted by the
 * reference's rule: m >= 5, inl / m >= ratioRansac, inl >= minPts, |t| < 3, |log R| < 1.5.  With m < 5: cand_inliers = 0 and cand_pose7 the
 * identity, as in an event.  Entries from n_candidates on: cand_kf = -1, zeros, the identity.
 * best: the accepted candidate with the most inliers, the earlier one in candidate order on a tie; then
 * T_c_map7 = cand_pose7[best] * T_c_w(cand_kf[best]) with the database's current pose (the one a pose graph corrected).  best = -1: the
 * identity.
 * No side effect a caller can observe: every later add_keyframes, process, poses, drift, similarity_row or keyframe call returns bit for
 * bit what it returns on a closer that never saw the query; a keyframe that was added and not yet processed stays pending.
 * FLVIS_ERR_INVALID_ARG before anything is queued: n_best outside 1 .. FLVIS_LC_FIX_CAND, a stream out of range or listed twice, n <= 0,
 * h_fix == NULL, a NULL closer; in the _host form (the checks and the staging of flvis_loop_closer_add_keyframes_host) wrong image shapes. */
#define FLVIS_LC_FIX_CAND 8
typedef struct flvis_lc_fix {
  int n_landmarks;   /* the query's kept ORB landmarks: what add_keyframes would have stored for it */
  int n_candidates;  /* <= n_best */
  int best;          /* index into cand_*; -1: not localised */
  int reserved;
  int64_t cand_kf[FLVIS_LC_FIX_CAND];
  double  cand_score[FLVIS_LC_FIX_CAND];
  int     cand_matches[FLVIS_LC_FIX_CAND], cand_inliers[FLVIS_LC_FIX_CAND], cand_accepted[FLVIS_LC_FIX_CAND];
  double  cand_pose7[FLVIS_LC_FIX_CAND][7]; /* as flvis_lc_event.loop_pose7: the query camera from keyframe cand_kf's camera */
  double  T_c_map7[7];                      /* best >= 0: the query camera's T_c_w in the map frame */
} flvis_lc_fix;
int flvis_loop_closer_localize(flvis_loop_closer* lc, int n, const int* h_stream, const uint8_t* d_img0, const void* d_img1,
                               int n_best, flvis_lc_fix* h_fix /* [n] */);
int flvis_loop_closer_localize_host(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0,
                                    const flvis_image* h_img1, int n_best, flvis_lc_fix* h_fix);
/* Localisation in ANOTHER sequence's map, or in all of them: flvis_loop_closer_localize with the searched database named per query.  (The
 * project's own, as localize is: the reference runs one sequence.)
 * Query: as in localize -- h_stream[i] (distinct) names the sequence whose camera took query i; the query goes through a keyframe's steps
 * with THAT sequence's camera (its P0 / P1 for the landmarks) into that sequence's query slot, and is not stored.
 * Searched map: h_map[i] is the sequence whose database is searched, FLVIS_LC_ALL_MAPS every sequence's, the query's own included.  Several
 * queries may name the same map.  An empty searched map gives n_candidates = 0, best = -1, map = -1, not an error.
 * Candidates: the n_best (1 .. FLVIS_LC_FIX_CAND) keyframes of the searched databases with score > 0 and >= prm.minScore, score descending,
 * equal scores by sequence ascending, then keyframe index ascending (flvis_hip_lc_select_maps' order: the global slot index).  No temporal
 * exclusion, no 50-keyframe gate.  Candidate r is keyframe fix.cand_kf[r] of sequence cand_seq[r].
 * Pair check per candidate: localize's, with side a the candidate's slot (its 3-D points, in the frame of the camera that stored it), side b
 * the query's slot (its pixels), and solvePnPRansac with the K of the QUERY's sequence -- the camera that saw the pixels.  The PnP seeds are
 * localize's ((h_stream[i] + 1) << 32 | rank + 1): with h_map[i] = h_stream[i] the result is localize's bit for bit.
 * Result: fix.best and ties as in localize; fix.T_c_map7 = cand_pose7[best] * T_c_w(cand_seq[best], cand_kf[best]), the query camera's pose
 * in the frame of map `map` = cand_seq[best].  Two uses: tying two maps, T_mapq_mapm = inv(T_c_mapq) * T_c_mapm from one frame localised
 * in both; joining a map, flvis_loop_closer_set_drift(q, inv(T_c_odom) * T_c_mapm).
 * No side effect a caller can observe on any sequence, as in localize.
 * Score rows: a device buffer of the call's own, [n_streams][max_keyframes] doubles from the first call on and
 * [n_streams][n_streams * max_keyframes] from the first call with FLVIS_LC_ALL_MAPS on (about 65 MB at 64 x 2000); when that allocation
 * fails the call returns FLVIS_ERR_HIP and the closer stays usable.  A closer that never makes the call allocates none of it.
 * FLVIS_ERR_INVALID_ARG before anything is queued: n_best outside 1 .. FLVIS_LC_FIX_CAND, a stream out of range or listed twice, an
 * h_map[i] outside -1 .. n_streams - 1, n <= 0, a NULL h_map, h_fix or closer; in the _host form wrong image shapes. */
#define FLVIS_LC_ALL_MAPS (-1)
typedef struct flvis_lc_fix_in {
  flvis_lc_fix fix;                /* as flvis_loop_closer_localize fills it; cand_kf[r] is an index within sequence cand_seq[r] */
  int cand_seq[FLVIS_LC_FIX_CAND]; /* the sequence whose database holds candidate r; -1 from n_candidates on */
  int map;                         /* cand_seq[fix.best]; -1 when not localised */
  int reserved;
} flvis_lc_fix_in;
int flvis_loop_closer_localize_in(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, const uint8_t* d_img0,
                                  const void* d_img1, int n_best, flvis_lc_fix_in* h_fix /* [n] */);
int flvis_loop_closer_localize_in_host(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, const flvis_image* h_img0,
                                       const flvis_image* h_img1, int n_best, flvis_lc_fix_in* h_fix);
/* Replaces the sequence's T_odom_map (the quaternion is normalised).  It enters the keyframes added afterwards
 * (T_c_w = T_c_w_odom * T_odom_map); stored poses, loops and the pose graph's trigger do not change, and a reset puts it back to the
 * identity.  A value that is not finite or a zero quaternion: FLVIS_ERR_INVALID_ARG and nothing changes.
 * The use it is for: after flvis_reset_streams on a tracker slot, localize the slot's first frame (tracker pose T_c_odom), set
 * T_odom_map = inv(T_c_odom) * T_c_map, and keep adding the slot's keyframes: they land in the map the sequence already has. */
int flvis_loop_closer_set_drift(flvis_loop_closer* lc, int stream, const double* h_T_odom_map7);
/* Merging sequences' maps: ONE pose graph over the keyframes of several sequences that have seen the same place.  (The project's own: the
 * reference runs one sequence.)
 * Link: ties keyframe kf_from of sequence seq_from to keyframe kf_to of sequence seq_to; pose7 is the `to` camera from the `from` camera, the
 * form of flvis_lc_event.loop_pose7 and flvis_lc_fix.cand_pose7 (its quaternion is normalised here).  An accepted candidate r of a
 * localize_in fix whose query frame was also stored as keyframe k of sequence q is the link (cand_seq[r], cand_kf[r]) -> (q, k), cand_pose7[r].
 * Group: the sequences h_seq[h_group_ptr[g] .. h_group_ptr[g + 1]), at least two, distinct; the first is the anchor, whose frame is the
 * merged map's.  Several disjoint groups go in one call and are optimised by one launch, one workgroup per group.
 * Joint graph of a group: flvis_hip_pgo_loop_closure with use_initial_guess = 1 on the virtual sequence
 *   rows:  the current T_c_w of every keyframe of the first sequence, 5 absent rows, every keyframe of the second sequence, 5 absent rows, ...
 *   loops: per sequence in group order its recorded loops in recorded order, shifted by the sequence's offset in the rows; then the group's
 *          links in the caller's order as (offset_from + kf_from, offset_to + kf_to).
 * Five absent rows cut the odometry chain, so only links tie the sequences; vertices, the fixed vertex, the edge order and the Cauchy /
 * Levenberg schedule are that call's.
 * Result per sequence s of a group, v_s its last keyframe that is a vertex (its last keyframe; in the group's last sequence the one at
 * max(later)): vertex rows get the optimised T_c_w, drift_s = inv(T_c_w_old(v_s)) * T_c_w_new(v_s), every keyframe behind v_s gets
 * T_c_w_old * drift_s (vo_loopclosing.cpp:922-925), and the sequence's T_odom_map becomes T_odom_map * drift_s: keyframes added afterwards
 * land in the merged frame.  Keyframes of the anchor before the first vertex stay as they are.  Nothing else changes: loop lists, the
 * pose-graph trigger, a pending unprocessed keyframe, similarity rows, the landmark database, and every sequence outside the groups.
 * The call keeps no links: the caller passes the whole list every time, and a second merge is another run on the current poses.
 * h_out[g]: whether group g's graph ran (always, for arguments that pass the checks), its vertices, edges, iterations and chi2 before / after.
 * h_drift7 (may be NULL): drift_s in the order of h_seq.
 * Buffers: the virtual sequences and the loop poses get device buffers of the call's own on its first use (and larger ones when a later call
 * needs them); when that allocation fails the call returns FLVIS_ERR_HIP and the closer stays usable.  A closer that never merges allocates none.
 * FLVIS_ERR_INVALID_ARG before anything is queued, and nothing changes: a NULL closer, h_group_ptr, h_seq, h_links or h_out; n_groups <= 0;
 * h_group_ptr that does not start at 0; a group of fewer than two sequences; a sequence out of range, or listed twice within or across groups;
 * an empty sequence in a group; a link whose sequences are not both in one group, whose two ends are in the same sequence, or whose `from`
 * sequence does not come before its `to` sequence in the group's order (the caller orders the group, no pose is inverted here); a keyframe
 * index outside its sequence; a pose7 that is not finite or has a zero quaternion; a non-anchor sequence that no chain of links connects to
 * the anchor; n_links < 0; iterations < 0. */
typedef struct flvis_lc_link {
  int seq_from, seq_to;
  int64_t kf_from, kf_to;
  double pose7[7];
} flvis_lc_link;
typedef struct flvis_lc_merge {
  int optimised, n_vertices, n_edges, iterations;
  double chi2_before, chi2_after;
} flvis_lc_merge;
int flvis_loop_closer_merge(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr /* [n_groups + 1] */, const int* h_seq,
                            int n_links, const flvis_lc_link* h_links, int iterations /* 100: the reference's */,
                            flvis_lc_merge* h_out /* [n_groups] */, double* h_drift7 /* [h_group_ptr[n_groups]][7], may be NULL */);
/* Links and loops from STORED keyframes: flvis_loop_closer_localize_in with a keyframe of the database as the query instead of images.  (The
 * project's own.)
 * Query: keyframe kf of sequence `stream` (-1: its newest).  Its own database slot is the query: no image, no feature kernel, nothing is
 * stored.  n >= 1 with no upper limit, and a sequence may appear any number of times (several of its keyframes, or one keyframe against
 * several maps).  A keyframe that was added and not yet processed is a valid query and stays pending.
 * Candidates: localize_in's rule over the searched map(s) -- `map`, or FLVIS_LC_ALL_MAPS -- minus what own_gap leaves out of the query's OWN
 * sequence: -1 all of it (with FLVIS_LC_ALL_MAPS: "all other maps"; with map == stream nothing is searched and n_candidates = 0, not an
 * error); g >= 0 its keyframes kf - g .. kf + g (0: only the query itself).  Keyframes of other sequences are never left out.
 * Pair check, acceptance, best, T_c_map7, map, cand_seq: localize_in's, with side a the candidate's slot, side b the query keyframe's slot,
 * the K of the QUERY's sequence and the PnP seeds (stream + 1) << 32 | rank + 1.  So for a keyframe that was stored from images I, a query
 * with map = m and own_gap = -1 returns bit for bit the fix that localize_in(stream, m, I) returns on the same closer.  T_c_map7 uses the
 * candidate's T_c_w as the database holds it at the time of the call (after merges and pose-graph runs).
 * Links: for every query in order and every accepted candidate r in rank order with cand_seq[r] != stream, the link {seq_from = cand_seq[r],
 * kf_from = cand_kf[r], seq_to = stream, kf_to = kf, pose7 = cand_pose7[r]} -- flvis_lc_links_from_fix's, ready for flvis_loop_closer_merge.
 * *n_links is the full count, at most link_cap are written (h_links may be NULL when link_cap = 0).  Accepted candidates in the query's own
 * sequence are loops, not links: they are in the fix only, and the sequence's loop list is not touched.
 * Any n: the queries run in passes of n_streams; a query's result does not depend on what else the call holds or on the call's order.
 * No side effect a caller can observe on any sequence, as in localize; the query slots of localize are not used.
 * Score rows: localize_in's buffer, allocated or grown as there; when that fails the call returns FLVIS_ERR_HIP and the closer stays usable.
 * FLVIS_ERR_INVALID_ARG before anything is queued, and nothing changes: n_best outside 1 .. FLVIS_LC_FIX_CAND, n <= 0, a stream or map out
 * of range, kf outside -1 .. count - 1 (so any kf on an empty sequence), own_gap < -1, link_cap < 0, link_cap > 0 with a NULL h_links, a
 * NULL h_q, h_fix, n_links or closer. */
typedef struct flvis_lc_link_query {
  int     stream;  /* the sequence that holds the query keyframe */
  int     map;     /* the sequence whose database is searched, or FLVIS_LC_ALL_MAPS */
  int64_t kf;      /* keyframe index in `stream`; -1: its newest */
  int64_t own_gap; /* what of the query's OWN sequence is left out: -1 all of it; g >= 0 the keyframes j with |j - kf| <= g */
} flvis_lc_link_query;
int flvis_loop_closer_link(flvis_loop_closer* lc, int n, const flvis_lc_link_query* h_q, int n_best, flvis_lc_fix_in* h_fix /* [n] */,
                           int link_cap, flvis_lc_link* h_links, int* n_links);
/* The links a localize_in (or link) fix yields when its query frame is keyframe kf of sequence `stream`: one per accepted candidate r in rank
 * order, {cand_seq[r], cand_kf[r]} -> {stream, kf} with cand_pose7[r]; candidates of sequence `stream` itself included (localize_in does
 * not leave them out).  Returns the count; at most cap are written (out may be NULL when cap = 0).  -1 for a NULL fix, cap < 0, or
 * cap > 0 with a NULL out.  Host only. */
int flvis_lc_links_from_fix(const flvis_lc_fix_in* fix, int stream, int64_t kf, int cap, flvis_lc_link* out);
/* The same link seen from its other end: the sequences and keyframes swapped, pose7 inverted (the quaternion is normalised first) -- what
 * flvis_loop_closer_merge needs when a link's `from` sequence comes after its `to` sequence in the group's order.  in == out is allowed.
 * FLVIS_ERR_INVALID_ARG for a NULL argument, a pose that is not finite or a zero quaternion.  Host only. */
int flvis_lc_link_reverse(const flvis_lc_link* in, flvis_lc_link* out);

/* ---- a map as points: landmarks of many keyframes in the map frame, one point per occupied voxel ---------------------------------------
 * (LocalMapNodeletClass publishes /map_cloud, vo_localmap.cpp:335-377 and :458-461, and sets up a pcl::VoxelGrid with an 0.08 m leaf that it
 * never runs: the raw cloud goes out.  leaf = 0 is that rounding; leaf > 0 is the filter, by this project's own rule.  This call is the
 * filter on caller arrays.  The local map's own cloud is flvis_local_map_cloud, which ends in this call; the loop closer's ORB landmarks
 * go through it as flvis_loop_closer_map_cloud -- a different map, of a nodelet the EuRoC launch does not load.)
 * Input: n_rows rows of up to cap points.  d_p3 [n_rows][cap][3] doubles in the row's camera frame; d_count [n_rows] (a negative count is
 * read as 0, one above cap as cap); d_T_c_w7 [n_rows][7] tx ty tz qx qy qz qw, the row's T_c_w.  A cloud is the concatenation of row
 * ranges: h_range2 [h_cloud_ptr[n_clouds]][2] = (first row, row count), cloud c owns the ranges h_cloud_ptr[c] .. h_cloud_ptr[c + 1].
 * A row may be in several ranges and several clouds.
 * Canonical order of a cloud's points: its ranges in the caller's order, rows ascending within a range, landmark index ascending.
 * Map-frame point: p = q_rotate(q_conj(q), p_c - t) on the pose as stored (dev_math.hpp; no normalisation), fp64 without contraction.  An
 *   identity pose returns p_c bit for bit (a zero coordinate comes out as +0).
 * Voxel index per axis: i = floor(p / leaf) in fp64 -- one correctly rounded division, then floor.  (PCL multiplies by a float inverse
 *   relative to the cloud's minimum: a point's voxel would depend on the other points.)
 * Dropped: a point with a coordinate that is not finite or an index outside -2^20 <= i < 2^20; counted in h_n_dropped.
 * Key: (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20).
 * leaf > 0: one output row per voxel that holds at least min_points points, rows ascending by key.  Per axis the row is the fp64 sum of the
 *   voxel's points -- the first point, then the others added one after another in canonical order -- divided by the count as a double and
 *   rounded once to float; d_npts is the count.
 * leaf == 0: no filter: every kept point in canonical order, rounded to float, d_npts = 1; min_points is not used.
 * Output: d_xyz [n_clouds][out_cap][3], d_npts [n_clouds][out_cap] (may be NULL), h_n_out [n_clouds] the FULL row counts -- at most out_cap
 *   rows are written per cloud, the first ones in output order; h_n_dropped [n_clouds] (may be NULL).  Rows from h_n_out on are not written.
 * Several clouds in one call give, cloud for cloud, the bits of as many single calls; a second run gives the same bits.
 * The call waits for its own counts (three times: the input points, which key bytes vary, the row counts) and for nothing else; d_xyz and
 *   d_npts are complete on the context's stream when it returns.
 * FLVIS_ERR_INVALID_ARG before anything is queued: leaf < 0 or not finite, min_points < 1, out_cap < 0, n_rows <= 0, cap <= 0, a range
 *   outside [0, n_rows), an h_cloud_ptr that does not start at 0 or decreases, n_clouds <= 0, a NULL d_p3, d_count, d_T_c_w7, h_cloud_ptr,
 *   h_range2 or h_n_out, a NULL d_xyz with out_cap > 0.  flvis_voxel_cloud_check is the host part of these checks on its own (no context).
 * FLVIS_ERR_CAPACITY: the clouds of the call hold 2^31 input points or more together (so: also a single cloud that does).
 * Workspace: the context's, grown on demand and kept: 48 bytes per input point of the call (two buffers of 64-bit keys and of 32-bit
 *   indices for the sort's passes, the fp64 map-frame point), 16 per listed row, 24 per cloud and a fixed 2.1 MB.  A failed allocation
 *   returns FLVIS_ERR_HIP and leaves the context usable.
 * Sort: stable LSD radix passes over 8-bit digits of (cloud index | key) in tiles of info[0] elements; a digit with one value in the
 *   whole call is skipped, and the cloud digits are skipped when no key digit ran or one cloud holds every point.
 * flvis_hip_voxel_cloud_info: h_info4 = sort tile (elements), workgroup size, workspace bytes per input point, per listed row.  Host only.
 * flvis_hip_voxel_cloud_stats: of the context's last call that got as far as the sort: passes run, passes skipped, workspace bytes the
 *   call needed, input points. */
int flvis_hip_voxel_cloud(flvis_ctx* ctx, const double* d_p3, const int* d_count, const double* d_T_c_w7, int n_rows, int cap, int n_clouds,
                          const int* h_cloud_ptr /* [n_clouds + 1] */, const int* h_range2, double leaf, int min_points, int out_cap,
                          float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped);
int flvis_voxel_cloud_check(int n_rows, int cap, int n_clouds, const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points,
                            int out_cap);
int flvis_hip_voxel_cloud_info(int* h_info4);
int flvis_hip_voxel_cloud_stats(flvis_ctx* ctx, int64_t* h_stats4);
/* The maps of a closer as voxel clouds: cloud g is flvis_hip_voxel_cloud over every stored keyframe of the sequences
 * h_seq[h_group_ptr[g] .. h_group_ptr[g + 1]) in that order, keyframes ascending -- one range per sequence over the landmark database
 * (camera-frame positions, counts) and the pose database.  Groups are written as flvis_loop_closer_merge takes them, but a group of one
 * sequence is allowed, a sequence may be in several groups, and only within a group the sequences must be distinct.
 * "Stored": everything add_keyframes has stored, processed or not (localize's database).  Each keyframe enters with the T_c_w the database
 * holds at the time of the call: after a merge of the same group the cloud is in the anchor's frame.  An empty sequence contributes
 * nothing; a group of empty sequences gives h_n_out = 0.
 * leaf, min_points, out_cap, d_xyz [n_groups][out_cap][3], d_npts (may be NULL), h_n_out, h_n_dropped (may be NULL): that call's.
 * _host: h_xyz / h_npts (may be NULL) are host arrays of the same shapes; the rows below min(h_n_out, out_cap) are written.
 * The call waits for its own counts (the _host form: and for its rows) and for nothing else.
 * No side effect a caller can observe: poses, drift, loops, similarity rows and events afterwards are bit for bit those of a closer that
 * never made the call; a keyframe that was added and not yet processed stays pending; the query slots of localize are not touched.
 * FLVIS_ERR_INVALID_ARG, and nothing changes: a NULL closer, h_group_ptr, h_seq or h_n_out; n_groups <= 0; an h_group_ptr that does not
 * start at 0 or decreases; a sequence out of range or twice in one group; the argument errors of flvis_hip_voxel_cloud. */
int flvis_loop_closer_map_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, double leaf, int min_points,
                                int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped);
int flvis_loop_closer_map_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, double leaf,
                                     int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped);

/* ---- whole trajectories in the map frame: every pose row, not only the keyframes ---------------------------------------------------------
 * (The reference broadcasts ONE tf map -> odom, the newest drift, vo_loopclosing.cpp:908: older poses shown through it are off by whatever
 * the pose graph has moved since.  Here every keyframe carries its own drift, and a row takes the drift of the keyframe it follows.)
 * pose7 = tx ty tz qx qy qz qw; the products are the closer's own (Hamilton q_mul, q_rot, pose_mul with its renormalisation), and
 *   pose_inv(T) = (-(R(q*) t), q*), q* = (-x, -y, -z, w).  fp64 without contraction, sqrt and / correctly rounded: every value is defined
 *   bit for bit.
 * Sequence s holds keyframes k = 0 .. n - 1 with O_k (the odometry pose it was added with, T_c_w_odom7), M_k (the stored pose, what
 *   flvis_loop_closer_poses returns) and a stamp tau_k, strictly increasing.  Keyframe drift: D_k = pose_mul(pose_inv(O_k), M_k).
 * Anchor of a row with stamp t: a = max{k : tau_k <= t}; a = 0 when t < tau_0; an empty sequence: a = -1 and D = h_drift7 of the sequence;
 *   a row whose stamp is NaN is copied unchanged, anchor -2.
 * FLVIS_LC_TRAJ_ANCHOR: D = D_a (for rows at or after the newest keyframe the reference's tf rule).
 * FLVIS_LC_TRAJ_BLEND: D = D_a when t < tau_0 or a = n - 1; else with u = (t - tau_a) / (tau_{a+1} - tau_a) and w0 = 1 - u the translation
 *   w0 * t_a + u * t_{a+1} and the quaternion w0 * q_a + (u * sigma) * q_{a+1}, sigma = -1 when dot(q_a, q_{a+1}) < 0 else 1, divided by
 *   the square root of its sum of squares (x, y, z, w summed in this order).  Continuous over a keyframe; no transcendental function:
 *   neighbouring drifts differ by what one pose graph spreads over a chain, where the chord is the geodesic to far below rounding.
 * Rows: FLVIS_LC_ROWS_POSE8 (t, T_c_w7) -> (t, pose_mul(T_c_w, D));  FLVIS_LC_ROWS_TRAJ9 (t, T_c_w7, state | new_kf << 4), a row of
 *   flvis_get_trajectory: the same, the last column copied, rows of every state;  FLVIS_LC_ROWS_IMU11 (t, qw qx qy qz, px py pz, vx vy vz),
 *   a row of flvis_get_imu_states, the body in the world frame: with E = pose_inv(D) the pose becomes pose_mul(E, (p, q)) and the velocity
 *   q_rot(E.q, v); w stays first.
 * flvis_hip_lc_map_poses is the call on caller arrays: d_T_odom, d_T_map [n_seq][kf_stride][7], d_stamps [n_seq][kf_stride], h_nkf [n_seq]
 *   the keyframes per sequence, h_drift7 [n_seq][7] (read for empty sequences; may be NULL when no job names one).  A job is n rows of one
 *   kind of one sequence: d_in, d_out [n][8 | 9 | 11], d_anchor [n] ints (may be NULL).  d_out == d_in is allowed (in place, the same
 *   pointer; any other overlap is the caller's error); a job with n == 0 is skipped; several jobs may name one sequence.  Rows need not be
 *   in order; a row's result does not depend on the others.  One upload, two launches (the drifts of the named sequences' keyframes, the
 *   rows), no atomics; the call returns synchronised with the context's stream.
 * FLVIS_ERR_INVALID_ARG, and no row is written: a mode or kind that does not exist, n_seq <= 0, a negative kf_stride, n_jobs or n, a
 *   keyframe count outside [0, kf_stride], a sequence out of range, a NULL h_nkf, h_jobs, d_in or d_out, a NULL table with a non-empty
 *   sequence named, and a named sequence whose stamps are not finite and strictly increasing (found on the device).  More than 65535 jobs:
 *   FLVIS_ERR_CAPACITY.  The context stays usable. */
enum { FLVIS_LC_TRAJ_ANCHOR = 0, FLVIS_LC_TRAJ_BLEND = 1 };
enum { FLVIS_LC_ROWS_POSE8 = 0, FLVIS_LC_ROWS_TRAJ9 = 1, FLVIS_LC_ROWS_IMU11 = 2 };
typedef struct flvis_lc_traj_job {
  int seq, kind, n;
  const double* d_in;
  double* d_out;
  int* d_anchor;
} flvis_lc_traj_job;
int flvis_hip_lc_map_poses(flvis_ctx* ctx, int n_seq, int kf_stride, const int* h_nkf, const double* d_T_odom /* [n_seq][kf_stride][7] */,
                           const double* d_T_map, const double* d_stamps, const double* h_drift7 /* [n_seq][7], for empty sequences */,
                           int n_jobs, const flvis_lc_traj_job* h_jobs, int mode);
/* The closer's keyframe stamps (host): unset (NaN) for a keyframe of flvis_loop_closer_add_keyframes[_host], KeyFrame.msg's header.stamp
 * for one of flvis_loop_closer_add_logged -- where that keeps the sequence's stamps strictly increasing: a log fed twice leaves the
 * second copy unset.  set: keyframes first_kf .. first_kf + n - 1 of the sequence; the stamps of a sequence must be finite and strictly
 * increasing where set, and a call that would break this (or names keyframes the sequence does not hold) returns FLVIS_ERR_INVALID_ARG
 * and changes nothing.  keyframe_stamps: as flvis_loop_closer_poses ([cap], *n_out = keyframes in the sequence).
 * flvis_loop_closer_reset[_rigs] forgets the slot's stamps. */
int flvis_loop_closer_set_keyframe_stamps(flvis_loop_closer* lc, int stream, int first_kf, int n, const double* h_stamps);
int flvis_loop_closer_keyframe_stamps(flvis_loop_closer* lc, int stream, double* h_stamps, int cap, int* n_out);
/* Rows of any number of sequences into the map frame by the rule above, with the closer's own tables: O_k as handed to add_keyframes,
 * M_k the pose database as it is now (after every pose graph, flvis_loop_closer_set_drift and flvis_loop_closer_merge: for a merged
 * group the rows come out in the anchor sequence's frame), tau_k the stamps, h_drift7 the sequences' T_odom_map.  Jobs as above with
 * seq = the sequence; _host: d_in / d_out / d_anchor are HOST arrays (staged through the context's workspace).  O_k and tau_k reach the
 * device here, only what was added since the sequence's last upload; add, process and merge do nothing for this call.
 * Every stored keyframe counts, processed or not, and a pending keyframe stays pending: poses, drift, loops, similarity rows and events
 * afterwards are bit for bit those of a closer that never made the call.
 * FLVIS_ERR_INVALID_ARG, and nothing is written: the argument errors above, and a job on a sequence that holds an unstamped keyframe
 * (flvis_last_error names the sequence and the keyframe). */
int flvis_loop_closer_map_poses(flvis_loop_closer* lc, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode);
int flvis_loop_closer_map_poses_host(flvis_loop_closer* lc, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode);
/* The tracker's own record into the map frame without a pose crossing to the host: rows first_frame .. first_frame + n_frames - 1 of the
 * trajectory record (flvis_get_trajectory's rows and range checks) of the streams h_stream [n], stream s <-> sequence s, as
 * FLVIS_LC_ROWS_TRAJ9 jobs.  The closer's context must hold the tracker (FLVIS_ERR_INVALID_ARG without one, or without a trajectory
 * record), whose n_streams, image_width, image_height and cam_type must be the closer's (FLVIS_ERR_CONFIG); waits for the tracker's queued
 * work.  d_out_rows9 [n][n_frames][9] (device), h_out_rows9 the same on the host, h_anchor [n][n_frames] (host): each may be NULL.  The
 * record itself is not changed. */
int flvis_loop_closer_map_trajectory(flvis_loop_closer* lc, int n, const int* h_stream, int first_frame, int n_frames, int mode,
                                     double* d_out_rows9, double* h_out_rows9, int* h_anchor);

/* ---- a dense map from depth keyframes: back-project, voxel-filter on the device ---------------------------------------------------------
 * (The reference's octomap feeder, src/octofeeder/octomap_feeder.cpp:18-80, turns the depth image of every /vo_kf message into a point
 * cloud in the camera frame and hands it to octomap with the keyframe's pose.  Here the cloud goes straight into the voxel filter of
 * flvis_hip_voxel_cloud, in the map frame, without the 24-byte camera-frame rows ever existing.)
 * Input: d_depth [n_img][h][w] uint16, rows tightly packed (the keyframe log's img1 on depth rigs); d_T_c_w7 [n_img][7], the images'
 *   T_c_w.  Clouds are concatenations of image ranges exactly as flvis_hip_voxel_cloud's row ranges: h_cloud_ptr [n_clouds + 1],
 *   h_range2 [h_cloud_ptr[n_clouds]][2] = (first image, image count); an image may be in several ranges and clouds.  One camera per
 *   RANGE: h_cam5 [ranges][5] = fx, fy, cx, cy, depth_factor.
 * Sampling (flvis_depth_cloud_params): the pixels u = u0 + i * step_u < u1, v = v0 + j * step_v < v1 of every listed image.
 * A sample -- the tracker's own depth rule and order of operations (recover3DPts_c_FromDepthImg as the frame chain evaluates it):
 *   raw is read as UNSIGNED 16 bit; z = (float)((double)raw / depth_factor); the sample is valid iff (double)z >= z_min and
 *   (double)z <= z_max; p_c = (((double)u - cx) * (double)z / fx, ((double)v - cy) * (double)z / fy, (double)z), evaluated left to right
 *   in fp64 without contraction.  An invalid sample is not a point: it is counted nowhere but in its absence from h_n_valid, and
 *   h_n_dropped keeps flvis_hip_voxel_cloud's meaning (a map-frame coordinate that is not finite or a voxel index outside +-2^20).
 * Canonical order of a cloud's points: its ranges in the caller's order, images ascending within a range, then the image's valid samples
 *   in raster order (v ascending, then u).
 * RESULT: bit for bit what flvis_hip_voxel_cloud returns for rows that hold each listed image's valid p_c in canonical order under that
 *   image's pose: the same transform, division-then-floor key, stable sort, sequential fp64 sums and rounding to float (both front ends
 *   put a point through one device function).  Several clouds in one call give the bits of as many single calls; a second run gives
 *   the same bits (the compaction is a wave64 ballot and prefix count with per-wave bases in LDS: no atomic decides a position).
 *   With an identity pose, leaf = 0, step_u = step_v = 7, v0 = h / 2 - 22, v1 = h / 2 + 21, z_min = 0.5 and z_max = 6.5 the rows are the
 *   points octomap_feeder.cpp:35-61 pushes into its cloud.
 * leaf, min_points, out_cap, d_xyz [n_clouds][out_cap][3], d_npts (may be NULL), h_n_out, h_n_dropped (may be NULL): that call's.
 *   h_n_valid [n_clouds] (may be NULL): the valid samples per cloud, the voxel call's input points.
 * The call waits for its own counts as the voxel call does and for nothing else.
 * FLVIS_ERR_INVALID_ARG before anything is queued: a step < 1; a window that is empty or not inside the image (u1 <= 0 / v1 <= 0 stand
 *   for the width / height); z limits that are not finite or z_min > z_max; a camera entry that is not finite or whose fx, fy or
 *   depth_factor is 0; w <= 0 or h <= 0; a NULL d_depth, d_T_c_w7, h_cam5 or prm; and the argument errors of flvis_hip_voxel_cloud with
 *   n_img for n_rows.  flvis_depth_cloud_check is the host part of these checks on its own (no context).
 * FLVIS_ERR_CAPACITY: 2^31 valid samples or more in one call (or as many listed images times row chunks).
 * Workspace: the context's, grown on demand and kept: flvis_hip_voxel_cloud's 48 bytes per VALID sample, 12 bytes per listed image and
 *   row chunk (a chunk is about 4096 samples of whole sampled rows), 16 per listed image, 24 per cloud and the fixed 2.1 MB.  A failed
 *   allocation returns FLVIS_ERR_HIP and leaves the context usable.  flvis_hip_voxel_cloud_stats reports a dense call like a voxel call.
 * flvis_hip_depth_cloud_times: enable != 0 makes the context's later dense calls wait once more, behind the sort, and keep the wall-clock
 *   milliseconds of their four stages; h_ms4 (may be NULL) = count, keys, sort, rows of the last such call. */
typedef struct flvis_depth_cloud_params {
  int u0, v0, u1, v1;   /* sampled window, half-open; u1 <= 0 / v1 <= 0: the image's width / height */
  int step_u, step_v;   /* >= 1: samples u = u0 + i * step_u < u1, v = v0 + j * step_v < v1 */
  double z_min, z_max;  /* metres, both inclusive */
} flvis_depth_cloud_params;
int flvis_hip_depth_cloud(flvis_ctx* ctx, const uint16_t* d_depth, const double* d_T_c_w7, int n_img, int w, int h, int n_clouds,
                          const int* h_cloud_ptr /* [n_clouds + 1] */, const int* h_range2, const double* h_cam5,
                          const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                          int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_depth_cloud_check(int n_img, int w, int h, int n_clouds, const int* h_cloud_ptr, const int* h_range2, const double* h_cam5,
                            const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap);
int flvis_hip_depth_cloud_times(flvis_ctx* ctx, int enable, double* h_ms4);
/* The keyframe log as dense clouds: cloud c holds the logged keyframes of stream h_stream[c] (a stream may be listed more than once) --
 * all of them, or with h_slice2 [n][2] = (first entry, count) the entries first .. first + count - 1 that are logged (a slice reaching
 * past the log is cut, a negative first or count is refused).  Each depth image enters with its logged T_c_w, read out of the record in
 * place, and with the intrinsics (P0) and depth_factor of the stream's OWN config (flvis_tracker_create_rigs).  No image is copied.
 * Waits for the tracker's queued work.  Changes nothing in the log or the tracker: a run that made the call equals one that did not, bit
 * for bit.  A stream with no entry gives h_n_out = 0.  The other arguments and the _host form: as flvis_loop_closer_map_cloud's.
 * FLVIS_ERR_CONFIG: the tracker is not a depth rig.  FLVIS_ERR_INVALID_ARG: no tracker, the log is off, n <= 0, a stream out of range,
 * a bad slice, NULL h_stream, prm or h_n_out, and the argument errors of flvis_hip_depth_cloud. */
int flvis_keyframe_log_depth_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                   double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
                                   int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_keyframe_log_depth_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                        double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                        int64_t* h_n_dropped, int64_t* h_n_valid);
/* The dense map in the closer's frame: groups are written as for flvis_loop_closer_map_cloud; cloud g holds, for each sequence s =
 * h_seq[e] of the group in order, the logged keyframes i = 0 .. min(logged(s), stored(s) - first) - 1 of the tracker's stream s, entry i
 * under the closer's STORED T_c_w of keyframe first + i, first = h_first_kf[e] (per listed sequence; NULL: 0, the case after one
 * flvis_loop_closer_add_logged into an empty closer).  So after process, flvis_loop_closer_set_drift or flvis_loop_closer_merge the cloud
 * is in the map or the anchor's frame.  The camera is the closer's config of the sequence.  The context and shape conditions are those of
 * flvis_loop_closer_add_logged (FLVIS_ERR_CONFIG, FLVIS_ERR_INVALID_ARG) and the rig must be a depth rig (FLVIS_ERR_CONFIG); a first
 * outside [0, stored(s)] is FLVIS_ERR_INVALID_ARG, like the group errors of flvis_loop_closer_map_cloud.  Waits for the tracker's queued
 * work.
 * No side effect a caller can observe: poses, drift, loops, similarity rows and events afterwards are bit for bit those of a closer that
 * never made the call; a keyframe that was added and not yet processed stays pending; the query slots of localize are not touched; the
 * log and the tracker are not changed. */
int flvis_loop_closer_dense_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                  const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                                  int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_loop_closer_dense_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                       const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* h_xyz,
                                       int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);

/* ---- dense stereo: a depth image from a rectified pair -----------------------------------------------------------------------------------
 * (The reference has no dense matcher; like the voxel filter this is the project's own definition.  It is integer arithmetic until one
 * fp64 division, so it is defined bit for bit; tests/_dense_stereo.py restates it in numpy.)
 * Input: d_img0, d_img1 [n_img][h][w] uint8, rows tightly packed, RECTIFIED: a point at column u of image 0 lies at column u - d of
 *   image 1, d >= 0 (the keyframe log's img0 / img1 on cam_type 0).  h_cam2 [n_cam][2] = (bf, depth_factor), n_cam 1 (every image) or
 *   n_img (image i: entry i): bf = focal length times baseline in pixel-metres (-P1[3] of a config), depth_factor the Z16 unit of
 *   flvis_hip_depth_cloud.
 * Output, either may be NULL: d_disp16 [n_img][h][w] uint16, the disparity in 1/16 px, 0 = invalid; d_z16 [n_img][h][w] uint16, the
 *   layout flvis_hip_depth_cloud reads, 0 = invalid.
 * Definition (flvis_dense_stereo_params: d_min, n_disp, agg_r, uniq, lr_tol), every step integer:
 *   census      c(u, v): the 62 comparisons neighbour < centre of the window 9 wide x 7 high, defined for 4 <= u <= w - 5,
 *               3 <= v <= h - 4 (the bit order cannot be observed)
 *   cost        H(u, v, d) = popcount(c0(u, v) ^ c1(u - d, v)), defined where both words are
 *   aggregate   A(u, v, d) = the sum of H(u + du, v + dv, d) over |du|, |dv| <= agg_r, defined iff every term is:
 *               u - d - agg_r >= 4, u + agg_r <= w - 5, v - agg_r >= 3, v + agg_r <= h - 4
 *   candidates  D(u, v) = the d of [d_min, d_min + n_disp) with A defined; best = the argmin of A over D, the lowest d among equals;
 *               the pixel is invalid if D is empty
 *   uniqueness  invalid if some d' of D with |d' - best| > 1 has A(d') * (100 - uniq) < A(best) * 100
 *   left-right  (lr_tol >= 0; -1: off) bestR = the argmin over d of A(u' + d, v, d) at u' = u - best, over the d of the same range for
 *               which that is defined, the lowest d among equals; invalid if |bestR - best| > lr_tol
 *   sub-pixel   best - 1 and best + 1 must both be in D(u, v), else invalid.  p = A(best - 1), n = A(best + 1), c = A(best),
 *               den = max(p + n - 2 c, 1): d16 = 16 best + floor(((p - n) * 16 + den) / (2 den)), the division rounding toward minus
 *               infinity.  d16 is the disparity output.
 *   depth       fp64, no contraction: z = (bf * 16.0) / (double)d16, raw = rint(z * depth_factor), ties to even; raw outside 1 .. 65535
 *               is invalid IN d_z16 ONLY (the disparity output keeps d16).
 * Several images in one call give the bits of as many single calls; a second run gives the same bits; no atomic decides a value.  An
 *   image too small to hold a valid pixel is no error: its outputs are all 0.
 * FLVIS_ERR_INVALID_ARG before anything is queued: n_disp < 1 or > 256; d_min < 0; d_min + n_disp > 4095 (16 d must fit 16 bits); agg_r
 *   outside 0 .. 4; uniq outside 0 .. 99; lr_tol < -1; w, h or n_img <= 0; n_cam neither 1 nor n_img; a camera entry that is not finite or
 *   not positive; both outputs NULL; a NULL image, h_cam2 or prm.  flvis_dense_stereo_check is the host part of these checks on its own
 *   (no context, no device: the device pointers are only compared with NULL).
 * No cost volume exists: a pair is read a small number of times through the cache and only the outputs are written.  Workspace, the
 *   context's, grown on demand and kept: with lr_tol >= 0 the right view's argmin, 2 bytes per pixel of min(n_img, 64) images (a call
 *   runs its images 64 at a time), and 16 bytes per camera.  A failed allocation returns FLVIS_ERR_HIP and leaves the context usable.
 *   The call queues its kernels and returns; it waits only for the upload of the cameras. */
typedef struct flvis_dense_stereo_params {
  int d_min;   /* >= 0: the first disparity searched */
  int n_disp;  /* 1 .. 256: the disparities d_min .. d_min + n_disp - 1 */
  int agg_r;   /* 0 .. 4: the box sum covers (2 agg_r + 1)^2 pixels */
  int uniq;    /* 0 .. 99, per cent */
  int lr_tol;  /* >= 0: the left-right tolerance in px; -1: no check */
} flvis_dense_stereo_params;
int flvis_hip_dense_stereo(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam,
                           const double* h_cam2, const flvis_dense_stereo_params* prm, uint16_t* d_disp16, uint16_t* d_z16);
int flvis_dense_stereo_check(const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam, const double* h_cam2,
                             const flvis_dense_stereo_params* prm, const uint16_t* d_disp16, const uint16_t* d_z16);

/* ---- the dense map on rectified stereo rigs: the keyframe log's pairs through flvis_hip_dense_stereo ------------------------------------
 * On stereo rigs the log keeps both working images of every keyframe; on cam_type 0 (the D435i infra pair, the pixhawk variant, KITTI)
 * the pair is rectified.  These calls put such pairs through flvis_hip_dense_stereo with bf = -P1[3] of the stream's (the sequence's) OWN
 * config and the caller's depth_factor (the Z16 unit of the intermediate depth image; 1000 = millimetres), and hand the Z16 images to
 * flvis_hip_depth_cloud.  cam_type 1 (EuRoC: the logged pair is NOT rectified and needs a remap in front: the flvis_*_unrect_stereo_* calls
 * below) and cam_type 2 (a depth rig: flvis_keyframe_log_depth_cloud) return FLVIS_ERR_CONFIG.  The depth-rig calls keep refusing stereo rigs.
 * flvis_keyframe_log_stereo_z16: the whole Z16 image of the entries (h_stream[i], h_index[i]), i < n, into d_z16 [n][h][w] (device, the
 *   caller's).  Waits for the tracker's queued work, queues the matcher and returns.  FLVIS_ERR_INVALID_ARG: no tracker, the log off,
 *   n <= 0, a NULL pointer, a stream out of range, an entry that is not logged, and the argument errors of flvis_hip_dense_stereo.
 * flvis_keyframe_log_stereo_cloud(_host), flvis_loop_closer_stereo_cloud(_host): the arguments and semantics of
 *   flvis_keyframe_log_depth_cloud(_host) and flvis_loop_closer_dense_cloud(_host) with the stereo parameters and depth_factor in front of
 *   the sampling.  RESULT: bit for bit flvis_hip_depth_cloud on the Z16 images flvis_keyframe_log_stereo_z16 gives for the same entries,
 *   with the intrinsics of P0, depth_factor, and the logged poses (the closer's stored poses), exactly as the depth-rig calls take them.
 *   The no-side-effect guarantees of the depth-rig calls hold: the log, the tracker and the closer are only read.
 * Workspace, the context's, grown on demand and kept: the matcher is evaluated on whole images, 64 at a time, but only the Z16 values AT
 *   THE CLOUD'S SAMPLES are kept: 2 bytes per sample (not per pixel) of every listed keyframe, 20 bytes per listed keyframe, the 2 bytes
 *   per pixel of 64 images of flvis_hip_dense_stereo's left-right map (39 MB at 640 x 480), and flvis_hip_depth_cloud's own workspace.
 *   27200 keyframes of 640 x 480 at step 7 (92 x 69 samples): 345 MB of samples.  A failed allocation returns FLVIS_ERR_HIP and leaves
 *   the context usable. */
int flvis_keyframe_log_stereo_z16(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, const flvis_dense_stereo_params* prm,
                                  double depth_factor, uint16_t* d_z16);
int flvis_keyframe_log_stereo_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                    double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                    float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_keyframe_log_stereo_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                         double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                         float* h_xyz, int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_loop_closer_stereo_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                   const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm, double leaf,
                                   int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped,
                                   int64_t* h_n_valid);
int flvis_loop_closer_stereo_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                        const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                        double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                        int64_t* h_n_dropped, int64_t* h_n_valid);

/* ---- rectification: raw, distorted images into rectified ones ----------------------------------------------------------------------------
 * (The reference never remaps an image -- it undistorts points -- so this is the project's own definition.  It is fp64 up to one rounding
 * and integer after that, so it is defined bit for bit; tests/_rectify.py restates it twice in numpy.)
 * Input: d_src [n_img][h][w] uint8, rows tightly packed.  h_cam21 [n_cam][21] doubles, a camera each: K = (fx, fy, cx, cy) the raw
 *   intrinsics, D = (k1, k2, p1, p2) the raw radtan distortion, R[9] row-major the rectifying rotation, Pn = (fx', fy', cx', cy') =
 *   (P[0], P[5], P[2], P[6]) of the rectified projection (a config's cam0_intrinsics, cam0_distortion, R0, P0, or cam1_*, R1, P1).
 *   n_cam is 1 (every image), or n_img with h_cam_of NULL (image i: camera i), or any count with h_cam_of [n_img] naming a camera per image.
 * Output: d_dst [n_img][h][w] uint8, and optionally (may be NULL) d_covered [n_img][h][w] uint8, 1 where the pixel is covered, else 0.
 * Definition, for output pixel (u, v): every operation fp64, in exactly this order, left to right, no fused multiply-add:
 *   x = (u - cx') / fx';  y = (v - cy') / fy'
 *   X = R[0]*x + R[3]*y + R[6];  Y = R[1]*x + R[4]*y + R[7];  W = R[2]*x + R[5]*y + R[8]          (R^T (x, y, 1))
 *   xp = X / W;  yp = Y / W
 *   r2 = xp*xp + yp*yp;  rad = 1 + k1*r2 + k2*r2*r2
 *   xd = xp*rad + 2*p1*xp*yp + p2*(r2 + 2*xp*xp);  yd = yp*rad + p1*(r2 + 2*yp*yp) + 2*p2*xp*yp
 *   mx = fx*xd + cx;  my = fy*yd + cy;  tx = mx*32;  ty = my*32
 *   uncovered if tx or ty is not finite or |tx| or |ty| >= 2^30; else ix = rint(tx), iy = rint(ty), ties to even;
 *   sx = ix >> 5 (arithmetic: a floor), ax = ix & 31, and likewise sy, ay;
 *   covered iff sx >= 0, sy >= 0, sx + (ax > 0) <= w - 1 and sy + (ay > 0) <= h - 1: every tap of non-zero weight lies in the image (an
 *   identity camera reproduces its image, last row and column included);
 *   covered: ((32-ax)(32-ay) I[sy][sx] + ax(32-ay) I[sy][sx+1] + (32-ax) ay I[sy+1][sx] + ax ay I[sy+1][sx+1] + 512) >> 10, a tap of weight
 *   0 not read; uncovered: 0.
 * Several images in one call give the bits of as many single calls; a second run gives the same bits.  One kernel, no map table in
 *   memory: a thread evaluates the map once and walks the run of images that share its camera, so list the images camera by camera.
 * FLVIS_ERR_INVALID_ARG before anything is queued: a non-positive size or count; a NULL d_src, d_dst or h_cam21; n_cam neither 1 nor n_img
 *   with h_cam_of NULL; a camera index out of range; a camera entry that is not finite, or fx, fy, fx' or fy' <= 0; d_dst or d_covered
 *   overlapping d_src (the call is a gather and cannot run in place).  flvis_rectify_check is the host part on its own (no context, no
 *   device: the device pointers are only compared with NULL and with each other).
 * Workspace, the context's: 168 bytes per camera, 12 per run and nothing per pixel.  The call queues its kernel and returns; it waits only
 *   for the upload of the cameras. */
int flvis_hip_rectify(flvis_ctx* ctx, const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of,
                      uint8_t* d_dst, uint8_t* d_covered);
int flvis_rectify_check(const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of,
                        const uint8_t* d_dst, const uint8_t* d_covered);

/* ---- the dense map on the unrectified stereo rig (cam_type 1, EuRoC): the logged pairs rectified, then as above --------------------------
 * The tracker's landmarks and poses on this rig are of the RECTIFIED camera 0 (undistortPoints with R0 / P0, triangulation with P0 / P1),
 * so a cloud back-projected from a rectified depth image with P0 under the logged pose lies in the frame of the sparse map.
 * flvis_keyframe_log_rectified_pair: the rectified pair of the entries (h_stream[i], h_index[i]), i < n, into d_img0 / d_img1 [n][h][w]
 *   (device, the caller's; either may be NULL, not both): flvis_hip_rectify with camera 0 = (cam0_intrinsics, cam0_distortion, R0, P0) and
 *   camera 1 = (cam1_*, R1, P1) of the stream's own config.  Waits for the tracker's queued work, queues the kernel and returns.
 * flvis_keyframe_log_unrect_stereo_z16, flvis_keyframe_log_unrect_stereo_cloud(_host), flvis_loop_closer_unrect_stereo_cloud(_host): the
 *   argument lists and semantics of their stereo_ namesakes.  RESULT: bit for bit flvis_hip_dense_stereo, then flvis_hip_depth_cloud
 *   (intrinsics of P0, bf = -P1[3], the caller's depth_factor, logged or stored poses), on the pairs flvis_keyframe_log_rectified_pair
 *   gives for the same entries.  The closer's form reads stored poses only, whether or not flvis_loop_closer_set_stereo_unrect is on.  The
 *   log, the tracker and the closer are only read.  cam_type 0 and cam_type 2 return FLVIS_ERR_CONFIG.
 * Uncovered pixels enter the matcher as 0; masking their depth is out of scope (the caller's sampling window crops them where it matters:
 *   with alpha 0 they are none of camera 0 and a sliver at camera 1's border on the stock EuRoC rig).
 * Workspace, the context's, grown on demand and kept: rectified pairs exist for one batch of 64 pairs at a time (46 MB at 752 x 480),
 *   whatever the number of listed keyframes; the rest is the stereo forms' own. */
int flvis_keyframe_log_rectified_pair(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, uint8_t* d_img0, uint8_t* d_img1);
int flvis_keyframe_log_unrect_stereo_z16(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, const flvis_dense_stereo_params* prm,
                                         double depth_factor, uint16_t* d_z16);
int flvis_keyframe_log_unrect_stereo_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                           double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                           float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_keyframe_log_unrect_stereo_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2,
                                                const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                                double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                                int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_loop_closer_unrect_stereo_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                          const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                          double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
                                          int64_t* h_n_dropped, int64_t* h_n_valid);
int flvis_loop_closer_unrect_stereo_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq,
                                               const int* h_first_kf, const flvis_dense_stereo_params* sprm, double depth_factor,
                                               const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* h_xyz,
                                               int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid);

/* ---- an occupancy map from depth keyframes: free space by a ray walk on the device -------------------------------------------------------
 * (The reference's octomap feeder, src/octofeeder/octomap_feeder.cpp:18-80, hands its cloud and the sensor pose to an octomap server, which
 * casts a ray to every point.  The reference itself has no occupancy code: the rule below is this project's own, defined bit for bit;
 * tests/_occupancy.py restates it twice in numpy.)
 * Inputs: d_depth, d_T_c_w7, n_img, w, h, the ranges (h_map_ptr [n_maps + 1], h_range2), one camera per RANGE (h_cam5), the sampling `prm`
 *   and the validity rule are flvis_hip_depth_cloud's, maps for clouds.  Every LISTING of an image is a SCAN of its own (an image listed
 *   twice is two scans); a map's scans are numbered 0, 1, .. in canonical order: ranges in the caller's order, images ascending in a range.
 * All arithmetic below is fp64 without contraction unless float is stated.
 * Ray: one per valid sample.  Its end p is the sample's map-frame point, q_rotate(q_conj(q), p_c - t) with flvis_hip_depth_cloud's p_c:
 *   bit for bit the point that call makes.  Its origin o is p_c = (0, 0, 0) through the same function (so o.x starts from 0.0 - t.x).
 * Voxel index per axis: floor(x / leaf), one division and a floor, leaf > 0.  With io, ie the index triples of o and p: the ray is DROPPED
 *   (counted in h_n_dropped and nowhere else) if any coordinate of o or p is not finite or any index is outside [-2^20, 2^20).
 * Walk (integer-bounded: rounding cannot make it miss its end): per axis a, rem[a] = |ie[a] - io[a]|, sgn[a] = ie[a] >= io[a] ? 1 : -1, and
 *   for the axes with rem[a] > 0
 *     tmax[a] = ((double)(io[a] + (sgn[a] > 0 ? 1 : 0)) * leaf - o[a]) / (p[a] - o[a]),   tdel[a] = leaf / fabs(p[a] - o[a]).
 *   The current cell c starts at io.  Exactly rem[0] + rem[1] + rem[2] steps follow.  A step picks, among the axes with rem[a] > 0 NOW, the
 *   one with the smallest tmax: the axes are looked at in the order x, y, z and a later axis replaces the pick only if its tmax is
 *   strictly less (<), so a tie goes to the lowest axis.  Then c[a] += sgn[a], rem[a] -= 1, tmax[a] = tmax[a] + tdel[a].  The walk ends in ie.
 * Cells of a ray: its FREE cells are the cell before every step (the origin's cell and every visited cell but the last); its HIT cell is
 *   ie.  A ray of zero steps has a hit and no free cell.
 * Observation: per scan and voxel at most one -- a hit if any ray of the scan ends in the voxel, else a miss if any ray of the scan has it
 *   as a free cell (octomap's insertPointCloud: one update per scan, occupied wins).
 * Value (float): l starts from the prior's value of the voxel, or 0.0f.  For every scan that observes the voxel, in scan order:
 *   l = l + (hit ? l_hit : l_miss) as one float addition, then l = l < l_min ? l_min : (l > l_max ? l_max : l).  The clamp makes the order
 *   matter; the scan order is the definition.
 * Output, per map m: one row per voxel that is observed or in the prior, ascending by key; key = (iz + 2^20) << 42 | (iy + 2^20) << 21 |
 *   (ix + 2^20) (flvis_hip_voxel_cloud's sort key) in d_key [n_maps][out_cap], the value in d_l [n_maps][out_cap], and in d_xyz
 *   [n_maps][out_cap][3] (may be NULL) the centre (float)(((double)i + 0.5) * leaf) per axis.  h_n_out [n_maps]: the full row count (at most
 *   out_cap rows are written); h_n_rays, h_n_dropped [n_maps] (may be NULL): rays cast and rays dropped.
 * Prior: map m may start from the first h_n_prior[m] rows of d_prior_key / d_prior_l [n_maps][prior_cap] (device; all of d_prior_key,
 *   d_prior_l, h_n_prior may be NULL and prior_cap 0: no prior).  A map's prior keys must ascend strictly and be non-negative: checked on
 *   the device.  That they are keys of the same leaf is the caller's contract.  The prior may not alias the output.  A prior voxel that no
 *   scan observes comes out unchanged.
 * Chaining: scans 0 .. k - 1 in one call, then scans k .. n - 1 with that call's output as prior, give bit for bit the map of one call over
 *   scans 0 .. n - 1 (the value rule is a left fold over the scans, and the prior stands for a scan before scan 0).
 * Reproducibility: several maps in one call give the bits of as many single calls; a second run gives the same bits.  No atomic decides a
 *   position or a value (positions are prefix sums; the "any hit" of a scan is an OR, which no order changes).
 * Method: every cell of every ray is a record (key, canonical index, scan << 1 | hit), written at its exact canonical position (map, scan,
 *   raster, step; a ray's record count |ie - io|_1 + 1 is known without walking, so positions are prefix sums of a count pass);
 *   flvis_hip_voxel_cloud's stable radix sort; then runs of one (voxel, scan) collapse to observations IN PARALLEL and one lane per voxel
 *   applies its observations (at most one per scan, plus the prior) in order.  The call waits for its counts, for the byte table of the
 *   sort and for the maps' row counts.
 * FLVIS_ERR_INVALID_ARG before anything is queued: leaf <= 0 or not finite; l_hit <= 0, l_miss >= 0, l_min >= 0, l_max <= 0 or any of them
 *   not finite; h_n_prior[m] outside [0, prior_cap]; a NULL prior table with a non-zero count; a prior that overlaps the output; NULL occ,
 *   or NULL d_key or d_l with out_cap > 0; and every argument error of flvis_hip_depth_cloud.  flvis_occupancy_check is the host part of
 *   these checks on its own (no context, no pointer checks of device arrays).  A prior whose keys do not ascend: FLVIS_ERR_INVALID_ARG after
 *   the device check, with no row written.
 * FLVIS_ERR_CAPACITY: 2^31 - 1 records or more in one call (prior rows count as records), known after the count pass, before the record
 *   buffers are allocated.
 * Workspace: the context's, grown on demand and kept: 32 bytes per record (two key and two index buffers of the sort, the payload, and the
 *   voxel rank of an observation; observations reuse the sort's second buffers), nothing per ray (a ray is derived from its sample in the
 *   count and in the emit pass, never stored), 20 bytes per listed image, 20 per listed image and row chunk, 44 per map and the sort's
 *   fixed tables.  flvis_hip_occupancy_info: h_info4 = workgroup size, workspace bytes per record, per ray, per listed image.  Host only.
 *   A failed allocation returns FLVIS_ERR_HIP and leaves the context usable.
 * flvis_hip_occupancy_stats: h_stats4 = records (prior rows included), rays, batches, workspace bytes of the context's last occupancy
 *   call; h_ms4 = wall-clock milliseconds of count, emit, sort, reduce, summed over the call's batches, kept while
 *   flvis_hip_depth_cloud_times is enabled (the call then waits behind every stage).  Either may be NULL. */
typedef struct flvis_occupancy_params {
  float l_hit, l_miss, l_min, l_max;  /* log-odds added per hit / miss observation, and the clamp */
} flvis_occupancy_params;
void flvis_occupancy_params_default(flvis_occupancy_params* p);  /* 0.85f, -0.4f, -2.0f, 3.5f: octomap's documented log-odds */
int flvis_hip_occupancy(flvis_ctx* ctx, const uint16_t* d_depth, const double* d_T_c_w7, int n_img, int w, int h, int n_maps,
                        const int* h_map_ptr /* [n_maps + 1] */, const int* h_range2, const double* h_cam5,
                        const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, const int64_t* d_prior_key,
                        const float* d_prior_l, int prior_cap, const int64_t* h_n_prior, int out_cap, int64_t* d_key, float* d_l, float* d_xyz,
                        int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped);
int flvis_occupancy_check(int n_img, int w, int h, int n_maps, const int* h_map_ptr, const int* h_range2, const double* h_cam5,
                          const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int prior_cap,
                          const int64_t* h_n_prior, int out_cap);
int flvis_hip_occupancy_info(int* h_info4);
int flvis_hip_occupancy_stats(flvis_ctx* ctx, int64_t* h_stats4, double* h_ms4);
/* The keyframe log as occupancy maps (depth rigs, cam_type 2; a stereo rig: FLVIS_ERR_CONFIG): map c holds the logged keyframes of stream
 * h_stream[c] as its scans, listed, posed and calibrated exactly as flvis_keyframe_log_depth_cloud lists them (h_slice2 included).
 * The scans are walked in BATCHES whose scan records stay at or below max_records (0: 2^26; negative: FLVIS_ERR_INVALID_ARG): one count
 * pass over every listed keyframe gives the records of every scan, read once; scans are taken in canonical order, map after map, while
 * they fit; each batch is one flvis_hip_occupancy over all maps with the map so far as the prior, carried in two buffers of the context
 * that a batch writes and the next reads.  By the chaining property the result is bit for bit the one-call result, and the workspace is
 * bounded by max_records and the size of the maps, not by the number of keyframes.  *h_n_batches (may be NULL): the batches run.  A single
 * scan above max_records: FLVIS_ERR_CAPACITY, the message names the stream and the entry.
 * No image leaves HBM, nothing is added to the frame chain, the log and the tracker are only read: a run that made the call equals one that
 * did not, bit for bit.  Outputs as flvis_hip_occupancy's, d_key / d_l / d_xyz [n][out_cap]; the _host form stages them in the context.
 * The closer's form: the groups, stored poses, cameras and conditions of flvis_loop_closer_dense_cloud, so after process,
 * flvis_loop_closer_set_drift or flvis_loop_closer_merge the map is in the map or the anchor's frame; no side effect on the closer. */
int flvis_keyframe_log_occupancy(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm, double leaf,
                                 const flvis_occupancy_params* occ, int64_t max_records, int out_cap, int64_t* d_key, float* d_l, float* d_xyz,
                                 int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped, int* h_n_batches);
int flvis_keyframe_log_occupancy_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                      double leaf, const flvis_occupancy_params* occ, int64_t max_records, int out_cap, int64_t* h_key, float* h_l,
                                      float* h_xyz, int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped, int* h_n_batches);
int flvis_loop_closer_occupancy(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int64_t max_records,
                                int out_cap, int64_t* d_key, float* d_l, float* d_xyz, int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped,
                                int* h_n_batches);
int flvis_loop_closer_occupancy_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                     const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int64_t max_records,
                                     int out_cap, int64_t* h_key, float* h_l, float* h_xyz, int64_t* h_n_out, int64_t* h_n_rays,
                                     int64_t* h_n_dropped, int* h_n_batches);

/* ---- occupancy map queries: the state of a voxel, and the first obstacle or unknown cell along a segment -----------------------------------
 * (An octomap consumer uses its map through search() and castRay(); these are the two calls for the maps above.  The rule is this
 * project's own, defined bit for bit; tests/_occupancy_cast.py restates it twice in numpy.)
 * A MAP is what the occupancy calls return: the first h_n_rows[m] rows of d_key [n_maps][map_cap] (int64) and d_l [n_maps][map_cap]
 *   (float), keys strictly ascending and non-negative, key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20), and ONE leaf for the
 *   whole call: that the keys belong to that leaf is the caller's contract, as it is for the prior.  Rows at and beyond h_n_rows[m] are
 *   never read.
 * A QUERY is a segment o -> p: six doubles (o.x o.y o.z p.x p.y p.z) in the map's frame, d_seg [n_q][6].  The queries of map m are
 *   h_q_ptr[m] .. h_q_ptr[m + 1] - 1 (CSR; a map may have none; n_q = h_q_ptr[n_maps]).
 * All arithmetic below is fp64 without contraction unless float is stated.
 * Cells: io, ie, rem, sgn, tmax, tdel, the order of the steps and the tie rule are word for word those of flvis_hip_occupancy:
 *   floor(x / leaf) per axis, exactly n = rem[0] + rem[1] + rem[2] steps, the step axis the one with the smallest tmax among the axes with
 *   rem[a] > 0, looked at in the order x, y, z with strict <.  The walk visits the cells c_0 = io, c_1, .., c_n = ie.  o and p are used as
 *   given: there is no pose and no camera.
 * Dropped: a query with a coordinate that is not finite, or with an index of io or ie outside [-2^20, 2^20), is DROPPED.
 * Entry parameter: t_0 = 0.0; for k >= 1, t_k is the value tmax[a] had when the step into c_k picked axis a, before tdel[a] was added.  It
 *   is reported as computed: rounding and the integer bound may take it a little past 1 or make it non-monotone; it is not corrected.
 * State of a cell: if its key is among the map's rows it is OCCUPIED when l > thres (one float comparison: l == thres is FREE, a NaN l is
 *   FREE) and FREE otherwise; if its key is absent it is UNKNOWN.
 * Walk: the cells are tested in the order k = 0, 1, ..  Before the test of cell k: if max_cells > 0 and k == max_cells, stop with LIMIT.
 *   Then the state of cell k decides: OCCUPIED: stop with OCCUPIED.  UNKNOWN and ignore_unknown == 0: stop with UNKNOWN.  Otherwise, if
 *   k == n: stop with END.  Otherwise step on.
 * Output per query (any of the arrays but d_status may be NULL): d_status int32 0 END, 1 OCCUPIED, 2 UNKNOWN, 3 DROPPED, 4 LIMIT; d_k int32
 *   the index of the cell where the walk stopped; d_cell int64 that cell's key; d_row int32 its row in the map, or -1 when it is absent or
 *   the status is LIMIT (a LIMIT cell is not looked up); d_l_out float the row's value, 0.0f when d_row is -1; d_t double t_k.  A DROPPED
 *   query gives k = 0, cell = -1, row = -1, l = 0.0f, t = 0.0.  h_counts5 [n_maps][5] (may be NULL): the queries per status.
 * Point lookup: a segment with p == o has n = 0; with ignore_unknown = 0 its status is END for free, OCCUPIED or UNKNOWN, and row / l are
 *   those of the point's voxel: that is search().
 * Reproducibility: queries are independent; several maps in one call give the bits of single calls; a second run gives the same bits.
 *   No atomics.
 * Method: one lane per query, in the caller's order.  The lane walks its segment with the integer-bounded walk of flvis_hip_occupancy
 *   and finds every cell's row in the map's sorted keys.  The keys of one (iz, iy) LINE share key >> 21 and lie together, ascending in
 *   ix, so each call first builds a LINE DIRECTORY per map: the distinct key >> 21 and the first row of each (head flags over the sorted
 *   keys, positions by prefix counts).  A lane keeps the row range of its current line and its place in it: after a step along x the next
 *   key is the old one +- 1 and its row, if any, is the neighbouring row (one load); after a step along y the next line is the old one
 *   +- 1 and its directory slot, if any, the neighbouring slot (one load), followed by a binary search inside that line; after a step
 *   along z a binary search over the directory on the side the step went to.  flvis_hip_occupancy_cast_lookup(ctx, 1) replaces all of
 *   that by one binary search over all rows of the map per cell (the baseline the directory is measured against; the same bits);
 *   0 is the default.  The call waits for the key check together with the line counts, and for the counts per status.
 * FLVIS_ERR_INVALID_ARG before anything is queued: leaf not finite or <= 0; thres not finite; max_cells < 0; ignore_unknown not 0 or 1;
 *   n_maps < 1; map_cap < 0 (an int: a capacity of 2^31 or more cannot be passed); h_n_rows[m] outside [0, map_cap]; h_q_ptr not
 *   starting at 0 or descending; NULL prm, h_n_rows or h_q_ptr; NULL d_key or d_l with a non-empty map; NULL d_seg or d_status with a query;
 *   an output that overlaps a map, the segments or another output.  flvis_occupancy_cast_check is the host part of these checks on its
 *   own (no context, no pointer checks of device arrays).  Map keys that do not ascend strictly, or a negative key:
 *   FLVIS_ERR_INVALID_ARG after a device check, with no output written.
 * FLVIS_ERR_CAPACITY: 2^31 - n_maps rows or more in the maps of one call (the directory holds ints).
 * Workspace: the context's, grown on demand and kept: 4 bytes per query, 64 per map, 4 per map and 256 rows of the largest map, and the
 *   directory, 12 bytes per row and per map (room for a line per row, so that its allocation waits for no count).  A failed allocation
 *   returns FLVIS_ERR_HIP and leaves the context usable.
 * flvis_hip_occupancy_cast_stats: h_stats4 = queries, cells tested, index bytes, workspace bytes of the context's last cast.  Cells
 *   tested: the sum of k + 1 over the queries that are not dropped, k for those that stopped with LIMIT; summed per map by a workgroup's
 *   tree, then over the maps.  Index bytes: the directory's lines and its head counts (0 with the plain search).  h_ms2 = wall-clock
 *   milliseconds of the index build (the key check, the line counts and the directory) and of the walk, kept while
 *   flvis_hip_depth_cloud_times is enabled (the call then waits behind the build).  Either may be NULL.
 * The _host form takes the segments from the host and returns the outputs there, staged in the context; the maps stay device arrays. */
typedef struct flvis_occupancy_cast_params {
  float thres;         /* a row is OCCUPIED when l > thres */
  int ignore_unknown;  /* 1: an UNKNOWN cell does not stop the walk */
  int max_cells;       /* > 0: stop with LIMIT before the test of cell max_cells */
} flvis_occupancy_cast_params;
void flvis_occupancy_cast_params_default(flvis_occupancy_cast_params* p);  /* 0.0f (probability 0.5), 0, 0 */
int flvis_hip_occupancy_cast(flvis_ctx* ctx, int n_maps, const int64_t* d_key, const float* d_l, int map_cap, const int64_t* h_n_rows,
                             double leaf, const flvis_occupancy_cast_params* prm, const double* d_seg, const int* h_q_ptr /* [n_maps + 1] */,
                             int* d_status, int* d_k, int64_t* d_cell, int* d_row, float* d_l_out, double* d_t, int64_t* h_counts5);
int flvis_hip_occupancy_cast_host(flvis_ctx* ctx, int n_maps, const int64_t* d_key, const float* d_l, int map_cap, const int64_t* h_n_rows,
                                  double leaf, const flvis_occupancy_cast_params* prm, const double* h_seg, const int* h_q_ptr, int* h_status,
                                  int* h_k, int64_t* h_cell, int* h_row, float* h_l_out, double* h_t, int64_t* h_counts5);
int flvis_occupancy_cast_check(int n_maps, int map_cap, const int64_t* h_n_rows, double leaf, const flvis_occupancy_cast_params* prm,
                               const int* h_q_ptr);
int flvis_hip_occupancy_cast_stats(flvis_ctx* ctx, int64_t* h_stats4, double* h_ms2);
int flvis_hip_occupancy_cast_lookup(flvis_ctx* ctx, int lookup);  /* 0 the line directory (default), 1 the plain search */

#ifdef __cplusplus
}
#endif
#endif /* FLVIS_HIP_H */
