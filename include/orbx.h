/*
 * orbx.h — C ABI of the MI355X-native ORB front-end (liborbx.so).
 *
 * Drop-in boundary for the ORB-SLAM2 hot path.  Plain C types
 * only; no OpenCV, no torch.  Every entry point names the reference interface
 * it replaces.  All functions return an orbx_status and never throw.
 *
 * Threading: a handle is single-threaded and owns one HIP stream plus its
 * device workspace (one extractor per thread, like the reference's left/right
 * extractors, src/Frame.cc:94-103).  The orbm_* matchers are re-entrant and
 * thread-safe: each synchronous host call runs on a non-blocking stream of its
 * own with pooled pinned / device buffers (no per-call device allocation, no
 * device-wide synchronisation), so concurrent callers (Tracking, LocalMapping,
 * LoopClosing) never wait on each other's or an extractor's stream.  Every
 * entry point leaves the calling thread's current HIP device as it found it.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ORBX_OK = 0,
    ORBX_EMPTY = 1,        /* empty input image: outputs untouched (src/ORBextractor.cc:1252) */
    ORBX_EINVAL = -22,
    ORBX_ENOMEM = -12,
    ORBX_EDEVICE = -5,
    ORBX_ENOSPC = -28      /* caller capacity too small */
} orbx_status;

/* Keypoints per frame the matcher searches take (SearchByBoW / SearchForTriangulation views and the
 * projection searches' frames): per-frame state of the greedy replays lives in a workgroup's LDS.  The
 * vocabulary transform takes up to ORBV_MAX_FEATURES descriptors per frame.  The reference has neither
 * limit (src/ORBmatcher.cc:45-129, 159-288; TemplatedVocabulary::transform); INTEGRATION.md §6. */
#define ORBM_MAX_FEATURES 16384
#define ORBV_MAX_FEATURES 65536

/* Layout-identical to cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;} */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

/* ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
 * include/ORBextractor.h:51-52; YAML keys ORBextractor.* (src/Tracking.cc:118-122). */
typedef struct {
    int nfeatures;
    float scale_factor;
    int nlevels;
    int ini_th_fast;
    int min_th_fast;
} orbx_params;

typedef struct orbx_handle orbx_handle;

/* Replaces ORBextractor::ORBextractor (src/ORBextractor.cc:466-540). device = HIP ordinal. */
orbx_status orbx_create(const orbx_params* params, int device, orbx_handle** out);
void orbx_destroy(orbx_handle* h);

/* Getters GetLevels/GetScaleFactor/GetScaleFactors/GetInverseScaleFactors/
 * GetScaleSigmaSquares/GetInverseScaleSigmaSquares (include/ORBextractor.h:63-83).
 * Each array has nlevels entries. Any pointer may be NULL. */
orbx_status orbx_get_tables(const orbx_handle* h, int* nlevels, float* scale_factor,
                            float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                            int* features_per_level);

/* OpenCV build the extractor reproduces.  The reference links whatever OpenCV 2.4 / 3.x
 * its user has (CMakeLists.txt:31-37), and the builds differ in the last bit of two primitives it calls:
 *   resize  cv::resize INTER_LINEAR's vertical pass in ComputePyramid (src/ORBextractor.cc:1361):
 *           ORBX_RESIZE_SCALAR  the generic FixedPtCast (h0 b0 + h1 b1 + 2^21) >> 22 (cv::setUseOptimized(false));
 *           ORBX_RESIZE_SSE2    x86 VResizeLinearVec_32s8u on all but a 0..4-px row tail (a stock x86 build).
 *   blur    GaussianBlur(7x7, 2) before computeDescriptors (src/ORBextractor.cc:1300-1306):
 *           ORBX_BLUR_SCALAR    OpenCV <= 3.4.1 integer column pass, kernel [18 34 49 55 49 34 18] / 2^8;
 *           ORBX_BLUR_SSE2      OpenCV <= 3.4.1 x86 SymmColumnVec_32s8u: the same sums rounded half to even on
 *                               every column but the row's width % 4 tail;
 *           ORBX_BLUR_BITEXACT  OpenCV >= 3.4.6 / 4.x fixed-point GaussianBlur, kernel [18 34 48 56 48 34 18] / 2^8.
 * The default is SCALAR / SCALAR, the path the CPU oracle pins.  DESIGN.md section 3 tabulates how far each mode
 * moves the output.  Takes effect from the next extract on the handle. */
enum { ORBX_RESIZE_SCALAR = 0, ORBX_RESIZE_SSE2 = 1 };
enum { ORBX_BLUR_SCALAR = 0, ORBX_BLUR_SSE2 = 1, ORBX_BLUR_BITEXACT = 2 };
orbx_status orbx_set_cv_modes(orbx_handle* h, int resize_mode, int blur_mode);

/* Per-frame keypoint capacity the extractor may need (nfeatures + slack per level).
 * -1 (and ORBX_EINVAL from the extract calls) for a geometry the kernels do not run:
 *   - a level narrower or shorter than one 30-px FAST cell inside its border (the
 *     reference divides by zero there, src/ORBextractor.cc:941-949);
 *   - a level whose quadtree region is less than half as wide as it is tall (nIni = 0,
 *     :650);
 *   - an image whose sides' bit widths sum to more than 24 (keypoint coordinates are packed in 24 bits,
 *     split between x and y by the image's shape: up to 4096 x 4096, 8192 x 2048, 16384 x 1024, ...);
 *   - a level whose resize source rows outgrow a workgroup's 160 KiB of LDS (sides above ~9,700 px).
 * Any keypoint budget runs: a level whose quadtree node list outgrows a workgroup's LDS
 * (about 1,700 keypoints, e.g. Tracking's 2 * nFeatures initialisation extractor at 4,000
 * features, src/Tracking.cc:133) keeps its node arrays in device memory instead. */
int orbx_capacity(const orbx_handle* h, int rows, int cols);

/* Replaces ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (include/ORBextractor.h:58-61, src/ORBextractor.cc:1248-1334).
 * Host image in, host keypoints/descriptors out (desc: cap x 32 bytes, row i
 * belongs to kps[i]).  Synchronous on the handle's stream.  Mask is ignored,
 * as in the reference.  The call's device work (upload, kernels, result copies)
 * is replayed as one hipGraph captured on the first call for an image size and
 * re-captured when the size changes; ORBX_NO_GRAPH=1 in the environment, or a
 * failed capture, falls back to direct launches with identical results. */
orbx_status orbx_extract(orbx_handle* h, const uint8_t* img, int rows, int cols, size_t step,
                         orbx_keypoint* kps, int cap, uint8_t* desc, int* n_out);

/* The public ORBextractor::mvImagePyramid (include/ORBextractor.h:85): level l of
 * the last orbx_extract, copied to host on the first call after each extract (cached
 * until the next one).  The level is unpadded (rows x cols bytes, pitch `step`); the
 * reference's level is a view inside a buffer with an EDGE_THRESHOLD = 19 px
 * BORDER_REFLECT_101 border (src/ORBextractor.cc:1352-1373), which copyMakeBorder of
 * this level rebuilds exactly (FetchPyramid). */
orbx_status orbx_get_level(orbx_handle* h, int level, const uint8_t** data, int* rows, int* cols,
                           size_t* step);

/* Batched device-resident replay (config 2/4): `batch` frames of rows x cols u8 at
 * d_imgs + f*frame_stride (row pitch `step`; frame_stride is not read when batch == 1), already in HBM.
 * Outputs per frame f:
 * d_kps[f*cap + i], d_desc[(f*cap + i)*32], d_counts[f].  Asynchronous on `stream`
 * (a hipStream_t taken literally: NULL is the HIP null stream). */
orbx_status orbx_extract_batch_device(orbx_handle* h, const uint8_t* d_imgs, int batch, int rows,
                                      int cols, size_t step, size_t frame_stride,
                                      orbx_keypoint* d_kps, uint8_t* d_desc, int* d_counts, int cap,
                                      void* stream);

/* The same extraction as orbx_extract_batch_device, issued one stage at a time so that a caller can
 * software-pipeline batches across streams (the VALU-bound FAST / describe stages of one batch beside
 * the latency-bound pyramid / quadtree stages of others).  stage 0: pyramid (and the counts reset),
 * 1: FAST, 2: quadtree (DistributeOctTree; writes d_counts), 3: describe (writes d_kps / d_desc).
 * Every stage takes the batch's full arguments and runs on its own `stream`; the caller orders the
 * four stages of a batch (events) and starts stage 0 of the handle's next batch only after stage 3 of
 * this one has completed (the stages share the handle's workspace).  Stage 0 sizes the workspace for
 * rows x cols x batch; later stages with other sizes return ORBX_EINVAL. */
orbx_status orbx_extract_stage_device(orbx_handle* h, int stage, const uint8_t* d_imgs, int batch, int rows,
                                      int cols, size_t step, size_t frame_stride, orbx_keypoint* d_kps,
                                      uint8_t* d_desc, int* d_counts, int cap, void* stream);

/* Wait for the work queued on `stream` (NULL = HIP null stream) and
 * return the device-side status (ORBX_ENOSPC when a frame exceeded `cap`). */
orbx_status orbx_sync(orbx_handle* h, void* stream);

/* Per-stage device timing (ms, HIP events recorded on the launch stream between
 * the stage kernels).  orbx_set_timing(h, 1) starts a new accumulation window;
 * orbx_get_stage_times returns the per-stage sums over every extract since then, host
 * (orbx_extract, launched directly instead of as a graph while timing is on), batched and
 * stage-split (orbx_extract_stage_device: each stage timed on its own stream).
 * Stages: 0 pyramid (all levels), 1 fast, 2 quadtree, 3 describe. */
orbx_status orbx_set_timing(orbx_handle* h, int enable);
orbx_status orbx_get_stage_times(orbx_handle* h, float* ms, int n);

/* Test hooks: device stage dumps of the last batch, frame f (host buffers).
 * pyramid: concatenated levels w_l*h_l; cand: per level (x_rel,y_rel,score) triples in
 * reference order (vToDistributeKeys); cand_counts[l]. */
orbx_status orbx_debug_pyramid(orbx_handle* h, int frame, uint8_t* out, size_t out_size);
orbx_status orbx_debug_candidates(orbx_handle* h, int frame, int level, int* xys, int cap, int* n);
/* Test hook: makes the bytes no kernel owns a test input.  Waits for the handle's last work, sets
 * every byte of the pyramid workspace and of the host path's staged input image (device block and
 * pinned staging rows), over their whole current capacity, to (uint8_t)value, and synchronises.
 * Buffers only grow, so the next extraction of a shape the workspace already holds keeps the fill
 * in every byte it does not write: the row padding of each level and the room past the last level. */
orbx_status orbx_debug_fill_workspace(orbx_handle* h, int value);
/* Kernel launches per stage of one batched extract of `batch` frames of rows x cols (measurement
 * hook: per-launch roofline figures): counts[0] pyramid, [1] FAST, [2] quadtree, [3] describe;
 * counts[4]: bit l set if a pyramid launch reads level l. */
orbx_status orbx_debug_launches(orbx_handle* h, int rows, int cols, int batch, int* counts, int n);
/* The quadtree form each level of one batched extract of `batch` frames of rows x cols runs (test hook;
 * launches nothing).  plan[8 * l ..]: workgroup size, keypoints per thread, 1 if the node arrays live in
 * global memory, 1 for the wide form (a side above 4096 px), node-list capacity, cell capacity, the bytes
 * the gather has for its owner map (it takes that path while 4 * cells + 2 * candidates fit), and the
 * index of the level's launch (levels of one launch share it).  `nlevels`: rows `plan` holds, at least
 * the extractor's level count. */
orbx_status orbx_debug_qt_plan(orbx_handle* h, int rows, int cols, int batch, int* plan, int nlevels);

/* ---- Stereo (Frame::ComputeStereoMatches, src/Frame.cc:630-872) ----
 * bf = Camera.bf (mbf), fx = K(0,0).  The search limits follow :676-681 with
 * mb = bf / fx (the value src/Frame.cc:140 assigns; the reference reads mb one
 * statement before that assignment).  Outputs mvuRight / mvDepth per left
 * keypoint (-1 = no stereo match) and the number of matches kept after the
 * median cut. */

/* Host path: `left` / `right` are the extractor handles (mpORBextractorLeft/Right)
 * right after their orbx_extract on the two images; kps/desc are what those calls
 * returned.  The SAD stage reads both handles' device pyramids (no pyramid D2H). */
orbx_status orbx_compute_stereo_matches(orbx_handle* left, orbx_handle* right, const orbx_keypoint* kps_l,
                                        const uint8_t* desc_l, int n_l, const orbx_keypoint* kps_r,
                                        const uint8_t* desc_r, int n_r, float bf, float fx, float* u_right,
                                        float* depth, int* n_good);

/* Batched device path (config 3): `npairs` stereo pairs of the handle's last
 * orbx_extract_batch_device batch, left frame d_left[p], right frame d_right[p]
 * (kps/desc/counts/cap as produced by that call; its level-0 images must still be
 * resident).  Outputs d_u_right[p*cap + i], d_depth[p*cap + i], d_n_good[p].
 * Asynchronous on `stream`. */
orbx_status orbx_stereo_batch_device(orbx_handle* h, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                     const int* d_counts, int cap, const int* d_left, const int* d_right,
                                     int npairs, float bf, float fx, float* d_u_right, float* d_depth,
                                     int* d_n_good, void* stream);

/* ---- Matcher (ORBmatcher Hamming inner loops, include/ORBmatcher.h:37-102) ---- */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1728-1744), host helper. */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);

enum { ORBM_TOP2 = 0, ORBM_FULL_U16 = 1 };

/* Config-5 brute force over device descriptors (32 B rows).  TOP2: per query the
 * first-min index and the best/second distances (SearchByBoW tie rule,
 * src/ORBmatcher.cc:214-224).  FULL_U16: the nq x nt distance matrix. */
orbx_status orbm_allpairs_device(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int mode,
                                 int* d_best_idx, int* d_best, int* d_second, uint16_t* d_full,
                                 void* stream);
/* The same on host arrays (SURVEY.md 8b orbm_allpairs), on HIP device `device`; synchronous.
 * nt == 0: TOP2 gives -1 / 256 / 256 per query. */
orbx_status orbm_allpairs(int device, const uint8_t* q, int nq, const uint8_t* t, int nt, int mode, int* best_idx,
                          int* best, int* second, uint16_t* full);

/* The inner loop every ORBmatcher search shares (SURVEY.md 8b orbm_best2_csr): query q's
 * candidates are d_cand_idx[d_cand_ptr[q] .. d_cand_ptr[q+1]) in the caller's visiting order (a
 * GetFeaturesInArea window, a FeatureVector node, ...).  tie_mode ORBM_TIE_FIRST keeps the first
 * candidate at the minimum distance (strict <, e.g. src/ORBmatcher.cc:214-224, 489-505);
 * ORBM_TIE_LAST the last one (dist > bestDist skip, SearchForTriangulation :806-823).  Outputs per
 * query: the best target index (-1 when the list is empty), its distance and the multiset second
 * distance (256 = none, the reference's initial value).  Candidate indices must lie in [0, nt).
 * Asynchronous on `stream`. */
enum { ORBM_TIE_FIRST = 0, ORBM_TIE_LAST = 1 };
orbx_status orbm_best2_csr_device(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, const int* d_cand_ptr,
                                  const int* d_cand_idx, int tie_mode, int* d_best_idx, int* d_best, int* d_second,
                                  void* stream);
/* Host arrays, on HIP device `device`; checks every candidate index.  Synchronous. */
orbx_status orbm_best2_csr(int device, const uint8_t* q, int nq, const uint8_t* t, int nt, const int* cand_ptr,
                           const int* cand_idx, int tie_mode, int* best_idx, int* best, int* second);

/* The coarse stage of Frame::ComputeStereoMatches alone (SURVEY.md 8b orbm_stereo_band,
 * src/Frame.cc:645-757), for callers that keep their own SAD refinement.  Per left keypoint: the right
 * keypoints whose row band [floor(y - 2*scale[o]), ceil(y + 2*scale[o])] holds the left row (int)y,
 * with octave within the left octave +- 1 and x in [xL - max_d, xL - min_d]; the first minimum of the
 * Hamming distance in increasing right index.  Outputs best_idx (-1 when no candidate is below
 * TH_HIGH = 100) and best_dist (100 then); the caller applies thOrbDist (:762).  Left keypoints with
 * y < 0, (int)y >= rows or xL - min_d < 0 get -1 / 100.  scale = the extractor's scale factors
 * (nlevels <= 32); right octaves must lie in [0, nlevels).  n_l, n_r <= 65535, and the row buckets
 * (4 * rows + 11 * cap bytes) must fit one workgroup's LDS (ORBX_ENOSPC otherwise). */
orbx_status orbm_stereo_band(int device, const orbx_keypoint* kps_l, const uint8_t* desc_l, int n_l,
                             const orbx_keypoint* kps_r, const uint8_t* desc_r, int n_r, int rows, const float* scale,
                             int nlevels, float min_d, float max_d, int* best_idx, int* best_dist);
/* Batched: pairs (d_left[p], d_right[p]) of a device batch (kps / desc / counts / cap as
 * orbx_extract_batch_device writes them); outputs d_best_idx[p*cap + i], d_best_dist[p*cap + i].
 * `scale` is a host array.  Asynchronous on `stream`. */
orbx_status orbm_stereo_band_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_counts, int cap,
                                    const int* d_left, const int* d_right, int npairs, int rows, const float* scale,
                                    int nlevels, float min_d, float max_d, int* d_best_idx, int* d_best_dist,
                                    void* stream);

/* The Frame grid (Frame's static members, src/Frame.cc:32-33): the image bounds of
 * Frame::ComputeImageBounds (src/Frame.cc:563-621; 0..cols x 0..rows without distortion, the
 * undistorted corners otherwise) and the FRAME_GRID_COLS x FRAME_GRID_ROWS = 64 x 48 cells over
 * them, mfGridElementWidthInv = 64.f / (mnMaxX - mnMinX) and HeightInv = 48.f / (mnMaxY - mnMinY)
 * in float (src/Frame.cc:127-128). */
typedef struct {
    float min_x, min_y;              /* mnMinX, mnMinY */
    float grid_w_inv, grid_h_inv;    /* mfGridElementWidthInv, mfGridElementHeightInv */
} orbm_grid;

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cc:417-588) for `npairs` frame pairs (F1 = pair_a[p], F2 = pair_b[p]) of an
 * `nframes` device batch in orbx_extract_batch_device's layout (kps/desc/counts, per-frame
 * capacity `cap`).  The keypoints are the frames' mvKeysUn (the extractor's own output for an
 * undistorted camera) in extractor order: level 0 first.  Candidates come from
 * F2.GetFeaturesInArea (src/Frame.cc:410-495) over `grid`.
 * d_prev_matched: vbPrevMatched per pair, d_prev_matched[(p*cap + i1)*2 + {0,1}] = (x, y), read as
 * the window centres and updated in place with F2's matched keypoint positions (:580-584), as
 * Tracking::MonocularInitialization keeps it across attempts (src/Tracking.cc:599-602, 639-644);
 * NULL = F1's own keypoint positions (the first attempt), not written.
 * Outputs: d_matches12[p*cap + i1] (-1 = none) and d_nmatches[p] (the return value).
 * cap <= 32767.  Pairs with more level-0 keypoints than one workgroup's LDS holds for the greedy
 * pass (about 43 bytes each, ~3,800) run it from device memory.  Asynchronous on `stream`. */
orbx_status orbm_search_for_initialization_device(const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                                  const int* d_counts, int nframes, int cap, const int* d_pair_a,
                                                  const int* d_pair_b, int npairs, const orbm_grid* grid,
                                                  int window, float nnratio, int check_ori, float* d_prev_matched,
                                                  int* d_matches12, int* d_nmatches, void* stream);

/* Host path for one (F1, F2) pair (host arrays), on HIP device `device`: kps1/desc1 = F1.mvKeysUn /
 * mDescriptors (n1), kps2/desc2 = F2's (n2), prev_matched = vbPrevMatched (n1 (x, y) pairs, in/out),
 * matches12 = vnMatches12 (n1), *nmatches = the return value.  nnratio / check_ori are the
 * ORBmatcher(nnratio, checkOri) arguments (Tracking uses 0.9, true).  Synchronous. */
orbx_status orbm_search_for_initialization(int device, const orbx_keypoint* kps1, const uint8_t* desc1, int n1,
                                           const orbx_keypoint* kps2, const uint8_t* desc2, int n2,
                                           const orbm_grid* grid, float* prev_matched, int window, float nnratio,
                                           int check_ori, int* matches12, int* nmatches);

/* The undistorted-camera shorthand of orbm_search_for_initialization_device: bounds 0..cols x
 * 0..rows and vbPrevMatched = F1's keypoints (the benchmark's replay of consecutive pairs). */
orbx_status orbm_search_init_batch_device(const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                          const int* d_counts, int nframes, int cap, const int* d_pair_a,
                                          const int* d_pair_b, int npairs, int rows, int cols,
                                          int window, float nnratio, int check_ori,
                                          int* d_matches12, int* d_nmatches, void* stream);

/* Test hook: what the SearchForInitialization launcher does for a call with per-frame capacity `cap`
 * and `npairs` pairs, computed by the function the launcher itself runs; host arithmetic only, no
 * kernel is launched.  out[10]: [0] query slices per pair of the top-4 build, [1] the number of
 * LDS-form greedy launches, [2..4] their level-0 capacities in ascending order (0 = unused),
 * [5] the device-memory greedy launch's capacity (0 = not launched), [6] the largest level-0 count
 * the LDS form holds, [7] the level-0 count up to which the grid is rank-sorted (counting sort
 * above), [8] the F2 grid count up to which the build stages F2 in LDS, [9] the queries one workgroup of
 * the build takes per sweep (a slice sweeps its pair's queries in steps of [0] * [9]). */
orbx_status orbm_debug_search_init_plan(int cap, int npairs, int* out);

/* ---- Vocabulary-node searches (SearchByBoW x2, SearchForTriangulation) ----
 * The candidate sets are the shared nodes of two DBoW2::FeatureVector maps
 * (std::map<NodeId, vector<unsigned>>, Thirdparty/DBoW2/DBoW2/FeatureVector.h),
 * passed as CSR: node ids ascending, the feature indices of node k at
 * fv_idx[fv_ptr[k] .. fv_ptr[k+1]) in insertion order.  Nodes hold disjoint
 * feature sets, so every shared node is one independent greedy search on the
 * device; the rotation-consistency filter runs per pair afterwards. */
typedef struct {
    const orbx_keypoint* kps;   /* n keypoints: mvKeysUn (KeyFrame) or mvKeys (Frame) */
    const uint8_t* desc;        /* n x 32 descriptors */
    const uint8_t* has_mp;      /* n flags (see the modes below); NULL = all 0 */
    const float* u_right;       /* n mvuRight values (triangulation); NULL = all -1 (monocular) */
    const int32_t* fv_node;     /* [fv_nnodes] ascending node ids */
    const int32_t* fv_ptr;      /* [fv_nnodes + 1] */
    const int32_t* fv_idx;      /* [fv_ptr[fv_nnodes]] feature indices */
    int32_t n;
    int32_t fv_nnodes;
} orbm_bow_view;

enum {
    /* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, ...), src/ORBmatcher.cc:159-288.
     * view1 = KF (has_mp = MapPoint present and !isBad), view2 = F.
     * match[iF] = KF feature whose MapPoint is assigned to F feature iF, -1 none. */
    ORBM_BOW_KF_F = 0,
    /* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, ...), :590-723.
     * has_mp = MapPoint present and !isBad on both sides.  match[idx1] = idx2. */
    ORBM_BOW_KF_KF = 1,
    /* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...), :725-891 (+ CheckDistEpipolarLine
     * :140-157).  has_mp = GetMapPoint(idx) != NULL.  match[idx1] = idx2 (vMatchedPairs). */
    ORBM_TRIANGULATION = 2
};

typedef struct {
    float F12[9];        /* fundamental matrix KF1 -> KF2, row-major */
    float ex, ey;        /* epipole of KF1's centre in KF2 (src/ORBmatcher.cc:731-736) */
    float scale2[16];    /* KF2 mvScaleFactors */
    float sigma2_2[16];  /* KF2 mvLevelSigma2 */
    int32_t only_stereo; /* bOnlyStereo */
} orbm_triang_params;

/* Batched device path: `npairs` searches; d_view1 / d_view2 / d_tp are device arrays of
 * the structs above whose pointers are device pointers (d_tp only for
 * ORBM_TRIANGULATION).  max_nodes1 >= every view1 fv_nnodes; every view2.n <= ORBM_MAX_FEATURES.  Outputs d_match[p *
 * match_stride + i] (i < view2.n for ORBM_BOW_KF_F, view1.n otherwise) and
 * d_nmatches[p].  nnratio = ORBmatcher::mfNNratio, check_ori = mbCheckOrientation.
 * Asynchronous on `stream`. */
orbx_status orbm_bow_search_device(int mode, const orbm_bow_view* d_view1, const orbm_bow_view* d_view2,
                                   const orbm_triang_params* d_tp, int npairs, int max_nodes1, float nnratio,
                                   int check_ori, int* d_match, int match_stride, int* d_nmatches, void* stream);

/* Host path for one pair (host pointers in the views and tp), run on HIP device `device`.
 * match: view2.n (ORBM_BOW_KF_F) or view1.n ints.  Synchronous. */
orbx_status orbm_bow_search(int device, int mode, const orbm_bow_view* view1, const orbm_bow_view* view2,
                            const orbm_triang_params* tp, float nnratio, int check_ori, int* match, int* nmatches);

/* ---- Projection search: ORBmatcher::SearchByProjection(Frame& F, vector<MapPoint*>, th) ----
 * src/ORBmatcher.cc:45-129, the local-map search of Tracking::SearchLocalPoints (src/Tracking.cc:1234-1244),
 * over Frame::GetFeaturesInArea (src/Frame.cc:410-495).  Per MapPoint, what Frame::isInFrustum left in it: */
typedef struct {
    float proj_x, proj_y, proj_xr;   /* mTrackProjX, mTrackProjY, mTrackProjXR */
    float view_cos;                  /* mTrackViewCos */
    int32_t level;                   /* mnTrackScaleLevel */
    int32_t flags;                   /* bit 0: mbTrackInView && !isBad(); bit 1: Observations() > 0 */
} orbm_proj_point;

typedef struct {
    float min_x, min_y;              /* Frame::mnMinX, mnMinY (image bounds, src/Frame.cc:563-621) */
    float grid_w_inv, grid_h_inv;    /* mfGridElementWidthInv / HeightInv */
    float th;                        /* the th argument */
    float nnratio;                   /* ORBmatcher::mfNNratio */
    float scale[16];                 /* F.mvScaleFactors */
} orbm_proj_params;

/* Batched device path: frame f has d_counts[f] keypoints (mvKeysUn), descriptors, mvuRight and
 * d_claimed (F.mvpMapPoints[i] && Observations() > 0) at f * cap; d_npts[f] MapPoints and their
 * descriptors at f * pcap.  Outputs d_match[f * cap + i] = the MapPoint (index) this call
 * assigned to feature i, -1 (the last one when it overwrote), and d_nmatches[f] (the
 * reference's return value).  cap <= ORBM_MAX_FEATURES.  Asynchronous on `stream`. */
orbx_status orbm_search_by_projection_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const float* d_uright,
                                             const uint8_t* d_claimed, const int* d_counts, int nframes, int cap,
                                             const orbm_proj_point* d_pts, const uint8_t* d_pdesc, const int* d_npts,
                                             int pcap, const orbm_proj_params* params, int* d_match,
                                             int* d_nmatches, void* stream);

/* Host path for one frame (host arrays), on HIP device `device`.  Synchronous. */
orbx_status orbm_search_by_projection(int device, const orbx_keypoint* kps, const uint8_t* desc, const float* uright,
                                      const uint8_t* claimed, int n, const orbm_proj_point* pts, const uint8_t* pdesc,
                                      int np, const orbm_proj_params* params, int* match, int* nmatches);

/* ---- Pose-projection searches: the other SearchByProjection overloads and Fuse ----
 * Each projects MapPoints with a camera pose and keeps, per MapPoint, the first minimum Hamming
 * distance over the GetFeaturesInArea window (Frame: src/Frame.cc:410-495, KeyFrame:
 * src/KeyFrame.cc:569-608):
 *   ORBM_PROJ_LAST_FRAME  SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 *                         src/ORBmatcher.cc:1396-1538 (Tracking::TrackWithMotionModel, src/Tracking.cc:937)
 *   ORBM_PROJ_KEYFRAME    SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist)
 *                         src/ORBmatcher.cc:1540-1667 (Tracking::Relocalization, src/Tracking.cc:1504,1518)
 *   ORBM_PROJ_SIM3        SearchByProjection(KeyFrame* pKF, Scw, vpPoints, vpMatched, th)
 *                         src/ORBmatcher.cc:290-403 (LoopClosing::ComputeSim3, src/LoopClosing.cc:375)
 *   ORBM_FUSE             Fuse(KeyFrame* pKF, vpMapPoints, th)            src/ORBmatcher.cc:893-1043
 *                         (LocalMapping::SearchInNeighbors, src/LocalMapping.cc:489,514)
 *   ORBM_FUSE_SIM3        Fuse(KeyFrame* pKF, Scw, vpPoints, th, vpReplacePoint)  src/ORBmatcher.cc:1045-1168
 *                         (LoopClosing::SearchAndFuse, src/LoopClosing.cc:599)
 * The three searches resolve the reference's in-call claims in MapPoint order (a feature taken
 * earlier in the call is skipped by later MapPoints) and apply the rotation histogram; the two
 * Fuse overloads make no claims during the search, so their per-MapPoint results are
 * independent and the caller applies Replace / AddObservation in MapPoint order. */
enum { ORBM_PROJ_LAST_FRAME = 0, ORBM_PROJ_KEYFRAME = 1, ORBM_PROJ_SIM3 = 2, ORBM_FUSE = 3, ORBM_FUSE_SIM3 = 4 };

typedef struct {
    float x, y, z;                /* MapPoint::GetWorldPos() */
    float nx, ny, nz;             /* GetNormal() (SIM3 and the Fuse modes) */
    float max_dist, min_dist;     /* mfMaxDistance, mfMinDistance (GetMax/MinDistanceInvariance's 1.2f / 0.8f applied inside) */
    float angle;                  /* LAST_FRAME: LastFrame.mvKeysUn[i].angle; KEYFRAME: pKF->mvKeysUn[i].angle */
    int32_t octave;               /* LAST_FRAME: LastFrame.mvKeys[i].octave */
    int32_t flags;                /* bit 0: take part -- LAST_FRAME: pMP && !mvbOutlier[i]; KEYFRAME: pMP && !isBad() &&
                                     !sAlreadyFound.count(pMP); SIM3 / FUSE_SIM3: !isBad() && not already found;
                                     FUSE: pMP && !isBad() && !IsInKeyFrame(pKF).  bit 1: Observations() > 0 */
    int32_t pad;
} orbm_map_point;

typedef struct {
    float fx, fy, cx, cy, bf, b;            /* intrinsics, mbf, mb */
    float min_x, max_x, min_y, max_y;       /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float grid_w_inv, grid_h_inv;           /* mfGridElementWidthInv / HeightInv */
    float log_scale;                        /* mfLogScaleFactor */
    int32_t nlevels;                        /* mnScaleLevels (1..16) */
    float th;                               /* the th argument */
    int32_t mono;                           /* bMono (LAST_FRAME) */
    int32_t orb_dist;                       /* ORBdist (KEYFRAME) */
    int32_t check_ori;                      /* ORBmatcher::mbCheckOrientation (LAST_FRAME, KEYFRAME) */
    float scale[16];                        /* mvScaleFactors */
    float inv_sigma2[16];                   /* mvInvLevelSigma2 (FUSE) */
} orbm_pose_params;

/* Batched device path.  Frame / KeyFrame f: d_counts[f] keypoints (mvKeysUn), descriptors,
 * mvuRight and d_claimed at f * cap (d_claimed[i] = the reference's "already taken" test on entry:
 * LAST_FRAME mvpMapPoints[i] && Observations() > 0; KEYFRAME mvpMapPoints[i]; SIM3 vpMatched[i];
 * ignored by the Fuse modes); d_pose[f * 24 ..]: row-major 3x4 mTcw (Scw for the SIM3 modes) then,
 * for LAST_FRAME, LastFrame.mTcw; d_npts[f] MapPoints and their descriptors at f * pcap.
 * Search modes: d_match[f * cap + i] = the MapPoint this call assigned to feature i (the last one),
 * -1 untouched, -2 set to NULL by the rotation filter; d_nmatches[f] = the reference's return value.
 * Fuse modes: d_match[f * pcap + m] = the feature MapPoint m fuses into (bestDist <= TH_LOW), -1;
 * d_nmatches[f] = nFused.  cap <= ORBM_MAX_FEATURES.  Asynchronous on `stream`. */
orbx_status orbm_project_search_device(int mode, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                       const float* d_uright, const uint8_t* d_claimed, const int* d_counts,
                                       int nframes, int cap, const float* d_pose, const orbm_map_point* d_pts,
                                       const uint8_t* d_pdesc, const int* d_npts, int pcap,
                                       const orbm_pose_params* params, int* d_match, int* d_nmatches, void* stream);

/* Host path for one Frame / KeyFrame (host arrays; pose = 24 floats as above), on HIP device
 * `device`.  match: n ints (search modes) or np ints (Fuse modes).  Synchronous. */
orbx_status orbm_project_search(int device, int mode, const orbx_keypoint* kps, const uint8_t* desc,
                                const float* uright, const uint8_t* claimed, int n, const float* pose,
                                const orbm_map_point* pts, const uint8_t* pdesc, int np,
                                const orbm_pose_params* params, int* match, int* nmatches);

/* ---- ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) ----
 * src/ORBmatcher.cc:1170-1394, called by LoopClosing::ComputeSim3 (src/LoopClosing.cc:323, th = 7.5) between
 * SearchByBoW(KF, KF) and SearchByProjection(pKF, Scw, ...).  Every feature of KF1 with a MapPoint that is not
 * in vpMatches12 yet goes to camera 1 (R1w, t1w), through sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 to camera
 * 2, and takes the first minimum Hamming distance over KeyFrame::GetFeaturesInArea(u, v, th * scale[level])
 * among octaves level-1..level, accepted at <= TH_HIGH (:1216-1293); the features of KF2 search KF1 through
 * sR12 = s12*R12, t12 (:1296-1373); a match stands where both directions agree (:1375-1391).
 * Both KeyFrames share one orbm_pose_params (the reference uses pKF1's intrinsics for both directions,
 * :1173-1176); of it only fx, fy, cx, cy, min/max_x/y, grid_*_inv, log_scale, nlevels, scale[] and th are
 * read.  Per feature an orbm_map_point holds GetMapPointMatches()[i]: x, y, z, max_dist, min_dist and flags
 * bit 0 = pMP && !pMP->isBad() (all else ignored), with pMP->GetDescriptor() as its descriptor.
 *
 * Batched device path.  nkf KeyFrames at stride cap: d_kps / d_desc (mvKeysUn, mDescriptors), d_mps /
 * d_mpdesc (GetMapPointMatches() per feature and each MapPoint's descriptor), d_counts[nkf],
 * d_pose[f * 12] row-major 3x4 Tcw.  Pair p: KF1 = d_pair_a[p], KF2 = d_pair_b[p], d_sim3[p * 13] = s12,
 * R12 (row-major), t12; d_already1[p * cap + i1] = vpMatches12[i1] != NULL on entry, d_already2[p * cap + i2]
 * = vbAlreadyMatched2[i2] (:1200-1210).  Outputs: d_match12[p * cap + i1] = the KF2 feature whose MapPoint
 * the call writes into vpMatches12[i1] (:1387), -1 where it writes nothing; d_nfound[p] = the return value;
 * d_match1 / d_match2 (NULL = not wanted): vnMatch1 / vnMatch2 before the agreement check (:1291, :1371).
 * Every output row has cap entries, -1 past the KeyFrame's count.  A pair whose s12 is not > 0 or whose
 * KeyFrame indices are outside [0, nkf) matches nothing.  cap <= ORBM_MAX_FEATURES.  Asynchronous on `stream`. */
orbx_status orbm_search_by_sim3_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const orbm_map_point* d_mps,
                                       const uint8_t* d_mpdesc, const int* d_counts, int nkf, int cap,
                                       const float* d_pose, const int* d_pair_a, const int* d_pair_b,
                                       const float* d_sim3, const uint8_t* d_already1, const uint8_t* d_already2,
                                       int npairs, const orbm_pose_params* params, int* d_match12, int* d_nfound,
                                       int* d_match1, int* d_match2, void* stream);

/* One pair, host arrays, on HIP device `device`; synchronous.  T1w / T2w: 12 floats (row-major 3x4 Tcw),
 * R12: 9 floats row-major, t12: 3.  match12 and match1: n1 ints, match2: n2 ints (match1 / match2 may be
 * NULL).  s12 must be > 0 and every keypoint octave in [0, 16). */
orbx_status orbm_search_by_sim3(int device, const orbx_keypoint* kps1, const uint8_t* desc1,
                                const orbm_map_point* mps1, const uint8_t* mpdesc1, const uint8_t* already1, int n1,
                                const float* T1w, const orbx_keypoint* kps2, const uint8_t* desc2,
                                const orbm_map_point* mps2, const uint8_t* mpdesc2, const uint8_t* already2, int n2,
                                const float* T2w, float s12, const float* R12, const float* t12,
                                const orbm_pose_params* params, int* match12, int* nfound, int* match1, int* match2);

/* ---- Image ingest ----
 * The per-frame preparation in front of ORBextractor::operator():
 *   cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) with the CV_32F maps of initUndistortRectifyMap and the
 *   default BORDER_CONSTANT 0 (Examples/Stereo/stereo_euroc.cc:97-98, 136-137), applied per channel, then
 *   cvtColor(CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) for 3- and 4-channel input
 *   (Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular, src/Tracking.cc:180-270).
 * Frame f: d_src + f * src_frame_stride, rows x cols, `channels` (1, 3, 4) interleaved u8, row pitch
 * src_step; rgb = Tracking::mbRGB.  Maps: NULL for no remap (dst_rows x dst_cols must equal rows x cols),
 * else nmaps pairs of dst_rows x dst_cols floats, frame f using pair f % nmaps (2 for a batch holding
 * L0 R0 L1 R1 ...).  Output: gray u8 at d_dst + f * dst_frame_stride, pitch dst_step -- the input
 * layout of orbx_extract_batch_device.  Asynchronous on `stream`. */
orbx_status orbx_ingest_batch_device(const uint8_t* d_src, int batch, int rows, int cols, int channels, int rgb,
                                     size_t src_step, size_t src_frame_stride, const float* d_map_x,
                                     const float* d_map_y, int nmaps, int dst_rows, int dst_cols, uint8_t* d_dst,
                                     size_t dst_step, size_t dst_frame_stride, void* stream);

/* GrabImageRGBD's imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (src/Tracking.cc:234-235; the caller
 * keeps the reference's condition for calling it).  depth_type 0: u16, 1: f32 input. */
orbx_status orbx_depth_batch_device(const void* d_src, int depth_type, int batch, int rows, int cols,
                                    size_t src_step, size_t src_frame_stride, float factor, float* d_dst,
                                    size_t dst_step, size_t dst_frame_stride, void* stream);

/* ---- Frame tail: what the Frame constructors do between the extractor and the matchers ----
 * (src/Frame.cc:145-197 RGB-D, :212-284 monocular; the stereo constructor's ComputeStereoMatches is above)
 * and Frame::isInFrustum of Tracking::SearchLocalPoints. */

/* mK and mDistCoef (CV_32F): Camera.fx .. Camera.k3 of the settings file (src/Tracking.cc:55-77). */
typedef struct { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } orbx_camera;

/* cv::undistortPoints(src, dst, K, D, noArray(), K) on n points (x, y float pairs): OpenCV 3.x's
 * cvUndistortPoints, 5 fixed-point iterations in double (unpinned against a real OpenCV).
 * Always undistorts, whatever k1 is.  xy_out may equal xy.  Pure host code, no device. */
orbx_status orbx_undistort_points(const orbx_camera* cam, const float* xy, int n, float* xy_out);

/* Frame::ComputeImageBounds (src/Frame.cc:587-621): bounds[4] = mnMinX, mnMaxX, mnMinY, mnMaxY, from the
 * undistorted corners (0,0) (cols,0) (0,rows) (cols,rows), or 0, cols, 0, rows when k1 == 0.  Pure host code. */
orbx_status orbx_image_bounds(const orbx_camera* cam, int rows, int cols, float* bounds);

/* Frame::UndistortKeyPoints (src/Frame.cc:539-579) over an extract batch ([nframes][cap] keypoints, d_counts):
 * mvKeysUn[i] = mvKeys[i] with pt undistorted; with k1 == 0.0 the keypoints are copied unchanged whatever the
 * other coefficients are (:543-547).  d_kps_un may equal d_kps; entries at and past d_counts[f] are not
 * written.  Asynchronous on `stream`. */
orbx_status orbx_undistort_batch_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                        const orbx_camera* cam, orbx_keypoint* d_kps_un, void* stream);

/* Frame::ComputeStereoFromRGBD (src/Frame.cc:875-896): d = imDepth.at<float>(kp.pt.y, kp.pt.x) at the
 * distorted keypoint, both coordinates truncated toward zero; d > 0: mvDepth = d, mvuRight = kpU.pt.x - mbf / d
 * (kpU = the undistorted keypoint), else both -1.  d_depth is the output layout of orbx_depth_batch_device:
 * frame f at d_depth + f * depth_frame_stride bytes (not read when nframes == 1), row pitch depth_step bytes.
 * Outputs d_uright[f * cap + i], d_depth_out[f * cap + i]; entries at and past d_counts[f] are not written.
 * Keypoints come from the extractor and lie inside rows x cols; one that does not (the reference reads out of
 * bounds there) gets -1 / -1.  Asynchronous on `stream`. */
orbx_status orbx_rgbd_stereo_batch_device(const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_un,
                                          const int* d_counts, int nframes, int cap, const float* d_depth,
                                          int rows, int cols, size_t depth_step, size_t depth_frame_stride,
                                          float bf, float* d_uright, float* d_depth_out, void* stream);

/* Host path for one frame (host arrays: n keypoints, a rows x cols float depth image of pitch depth_step bytes),
 * on HIP device `device`.  ORBX_EINVAL for a keypoint outside the image.  Synchronous. */
orbx_status orbx_rgbd_stereo(int device, const orbx_keypoint* kps, const orbx_keypoint* kps_un, int n,
                             const float* depth, int rows, int cols, size_t depth_step, float bf, float* uright,
                             float* depth_out);

/* Frame::isInFrustum(pMP, viewingCosLimit) (src/Frame.cc:342-398) as Tracking::SearchLocalPoints calls it
 * (src/Tracking.cc:1203-1230, limit 0.5): d_npts[f] MapPoints of frame f at f * pcap, d_pose[f * 12] = row-major
 * 3x4 mTcw.  Of an orbm_map_point it reads x, y, z, nx, ny, nz, max_dist, min_dist and flags (bit 0: the
 * caller's !isBad() && mnLastFrameSeen != mnId; bit 1: Observations() > 0); of params fx, fy, cx, cy, bf,
 * min/max_x/y, log_scale and nlevels.  Writes the orbm_proj_point array orbm_search_by_projection_device reads:
 * a point in view gets mTrackProjX / Y / XR, mTrackViewCos, mnTrackScaleLevel and flags = 1 | (flags & 2); a
 * point out of view, or one with bit 0 clear, all zero but flags = flags & 2.  d_ninview[f] = the number of
 * points with mbTrackInView set (nToMatch).  Entries at and past d_npts[f] are not written.  Asynchronous on
 * `stream`. */
orbx_status orbm_frustum_batch_device(const orbm_map_point* d_pts, const int* d_npts, int nframes, int pcap,
                                      const float* d_pose, const orbm_pose_params* params, float viewing_cos_limit,
                                      orbm_proj_point* d_out, int* d_ninview, void* stream);

/* Host path for one frame (host arrays; pose = 12 floats, row-major 3x4 mTcw), on HIP device `device`.
 * Synchronous. */
orbx_status orbm_frustum(int device, const orbm_map_point* pts, int np, const float* pose,
                         const orbm_pose_params* params, float viewing_cos_limit, orbm_proj_point* out,
                         int* ninview);

/* ---- Optimizer::PoseOptimization(Frame*) ----
 * src/Optimizer.cc:239-451: the motion-only bundle adjustment Tracking runs after every search (TrackReferenceKeyFrame
 * src/Tracking.cc:827, TrackWithMotionModel :950, TrackLocalMap :992, Relocalization :1492-1523), with the g2o pieces
 * it instantiates (Levenberg, BlockSolver_6_3, LinearSolverDense, the two OnlyPose edges, Huber, SE3Quat) restated on
 * the device; its arithmetic order is fixed in DESIGN.md §3.  One workgroup per frame.
 *
 * Inputs, as the searches leave them: d_kps (mvKeysUn; x, y and octave are read), d_uright (mvuRight: < 0 makes the
 * edge monocular, else stereo) and d_frame_mp (mvpMapPoints as indices into d_pts, -1 none) at f * fcap,
 * d_fcounts[f] features; of an orbm_map_point x, y, z and flags bit 1 (Observations() > 0); of params fx, fy, cx,
 * cy, bf, nlevels and inv_sigma2[]; d_pose_in[f * pose_stride] = row-major 3x4 mTcw, pose_stride 12 or 24 (the
 * d_pose of orbm_project_search_device).
 * Outputs: d_pose_out[f * 12] the optimised mTcw (the input pose where fewer than 3 features have a MapPoint; it
 * may alias no input); d_outlier[f * fcap + i] = mvbOutlier[i], written for the features with a MapPoint only;
 * d_ninliers[f] the return value (nInitialCorrespondences - nBad, 0 below 3 correspondences); d_trace[f] (may be
 * NULL) per round the outer iterations run, the rejected Levenberg trials and nBad, the rounds run and
 * nInitialCorrespondences; d_status[f] 0 or ORBM_POSE_OPT_INVALID.
 * With ORBM_POSE_OPT_DISCARD the call also runs the loop that follows the optimiser in TrackReferenceKeyFrame and
 * TrackWithMotionModel (src/Tracking.cc:830-848, :953-972): an outlier's d_frame_mp[i] becomes -1, its MapPoint index
 * goes to d_frame_outlier[f * fcap + i] (else -1; the array orbm_local_map_device takes), its flag is cleared, and
 * d_nmatches_map[f] counts the remaining features whose MapPoint has Observations() > 0.  Without the flag
 * d_frame_mp is only read, d_frame_outlier may be NULL and d_nmatches_map[f] counts the same set among the
 * non-outliers (mnMatchesInliers of TrackLocalMap, :1002-1020, outside localisation mode).  IncreaseFound,
 * mbTrackInView and mnLastFrameSeen stay with the caller.
 * Invalid: a count outside [0, fcap], a d_frame_mp entry outside [-1, nmp), an octave of a feature with a MapPoint
 * outside [0, nlevels).  Of an invalid frame only d_status[f] is written.  Entries at and past d_fcounts[f] are not
 * written.  fcap <= ORBM_MAX_FEATURES.  ORBX_EINVAL for a null or misaligned argument, an unknown flag and a
 * pose_stride other than 12 or 24.  Allocates nothing; asynchronous on `stream`. */
enum { ORBM_POSE_OPT_DISCARD = 1 };   /* flags */
enum { ORBM_POSE_OPT_INVALID = 1 };   /* d_status bits */

typedef struct {
    int32_t iters[4];      /* SparseOptimizer::optimize's iterations of each round */
    int32_t rejected[4];   /* Levenberg trials rejected and popped */
    int32_t nbad[4];       /* nBad after the round's classification */
    int32_t rounds;        /* rounds run: 0 (fewer than 3 correspondences), 1 (fewer than 10 edges) or 4 */
    int32_t ncorr;         /* nInitialCorrespondences */
} orbm_pose_opt_trace;

orbx_status orbm_pose_optimization_device(const orbx_keypoint* d_kps, const float* d_uright, const int* d_fcounts,
                                          int nframes, int fcap, int* d_frame_mp, const orbm_map_point* d_pts,
                                          int nmp, const float* d_pose_in, int pose_stride,
                                          const orbm_pose_params* params, int flags, float* d_pose_out,
                                          uint8_t* d_outlier, int* d_frame_outlier, int* d_ninliers,
                                          int* d_nmatches_map, orbm_pose_opt_trace* d_trace, int* d_status,
                                          void* stream);

/* Host path for one frame (host arrays: n features, nmp MapPoints, pose_in and pose_out 12 floats; frame_mp, outlier
 * and frame_outlier are updated in place as above), on HIP device `device`.  Synchronous. */
orbx_status orbm_pose_optimization(int device, const orbx_keypoint* kps, const float* uright, int n, int* frame_mp,
                                   const orbm_map_point* pts, int nmp, const float* pose_in,
                                   const orbm_pose_params* params, int flags, float* pose_out, uint8_t* outlier,
                                   int* frame_outlier, int* ninliers, int* nmatches_map, orbm_pose_opt_trace* trace,
                                   int* status);

/* Test hooks, not part of the interface a caller builds on (they may change or go without notice).
 * orbm_pose_optimization_host: the kernel's own code compiled for the CPU and run by one lane, the same arguments and
 * results without a device; tests/test_pose_optimization.py compares it with its restatement bit for bit. */
orbx_status orbm_pose_optimization_host(const orbx_keypoint* kps, const float* uright, int n, int* frame_mp,
                                        const orbm_map_point* pts, int nmp, const float* pose_in,
                                        const orbm_pose_params* params, int flags, float* pose_out, uint8_t* outlier,
                                        int* frame_outlier, int* ninliers, int* nmatches_map,
                                        orbm_pose_opt_trace* trace, int* status);

/* Test hook: sin, cos and the cube of theta as the pose optimiser's SE3 exponential evaluates them (out3[0..2]). */
void orbx_po_sincos_theta3(double theta, double* out3);

/* ---- MapPoint refresh: ComputeDistinctiveDescriptors and UpdateNormalAndDepth ----
 * src/MapPoint.cc:242-307 and :330-371, which the reference runs for every MapPoint of the KeyFrame concerned
 * after a KeyFrame insertion, a Fuse and a bundle adjustment (src/LocalMapping.cc:152-153, 442-444, 526-527,
 * src/Tracking.cc:554-555, 720-721, 1169-1170, src/Optimizer.cc:227, 776, 1042, src/LoopClosing.cc:500, 532,
 * src/MapPoint.cc:212).  They produce what every projection matcher above reads of an orbm_map_point -- nx, ny,
 * nz, max_dist, min_dist -- and its GetDescriptor().  One call refreshes np MapPoints in place.
 *
 * KeyFrame table: the layout of orbm_search_by_sim3_device (d_kps = mvKeysUn, d_desc = mDescriptors, d_counts,
 * cap, d_pose[f * 12] = row-major 3x4 Tcw) plus d_kf_bad[f] = pKF->isBad().  MapPoint m's mObservations are
 * d_obs[d_obs_ptr[m] .. d_obs_ptr[m + 1]) as (KeyFrame slot, feature index), in the order the caller's
 * std::map<KeyFrame*,size_t> iterates them: that order decides ties between medians and the order of the float
 * sum, and is never changed.  d_ref[m] = (mpRefKF's slot, mObservations[mpRefKF]).  Of params only nlevels and
 * scale[] are read (pRefKF->mnScaleLevels, mvScaleFactors).
 *
 * ORBM_REFRESH_DESCRIPTOR: among the observations whose KeyFrame is not bad, the descriptor with the least
 * median Hamming distance to all of them (element (int)(0.5*(N-1)) of its sorted row, its own 0 included; the
 * first row with the strictly smallest median) goes to d_pdesc[m], and its position in the point's full
 * observation list, bad KeyFrames counted, to d_best[m].  With no good KeyFrame d_pdesc[m] is left as it was.
 * ORBM_REFRESH_NORMAL_DEPTH, over all observations, bad KeyFrames included as in the reference: nx, ny, nz = the
 * mean of (Pos - Ow_i) / |Pos - Ow_i| summed in list order; max_dist = |Pos - Ow_ref| * scale[octave of the
 * ref keypoint]; min_dist = max_dist / scale[nlevels - 1].  A point on a camera centre gets a NaN normal.
 *
 * d_best[m]: >= 0 the winner (only when ORBM_REFRESH_DESCRIPTOR wrote d_pdesc[m]); -1 no descriptor written:
 * not selected, no good KeyFrame, or the point was skipped -- flags bit 0 clear (mbBad) or an empty list, where
 * nothing of the point is written; -2 the reference would read out of bounds and nothing of the point is written:
 * an observation or the ref with kf outside [0, nkf) or idx outside [0, min(d_counts[kf], cap)), the ref keypoint's
 * octave outside [0, nlevels), a list longer than max_obs or of negative length.  These are checked whatever
 * `what` selects.  Fields not selected, x, y, z, angle, octave, flags and pad always, and entries at and past np
 * keep their bits.  max_obs in [1, ORBM_MAX_OBSERVATIONS] is the caller's bound on a list's length and sizes the
 * LDS.  Asynchronous on `stream`. */
typedef struct { int32_t kf, idx; } orbm_observation;
enum { ORBM_REFRESH_DESCRIPTOR = 1, ORBM_REFRESH_NORMAL_DEPTH = 2 };
#define ORBM_MAX_OBSERVATIONS 1024

orbx_status orbm_refresh_map_points_device(int what, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                           const int* d_counts, int nkf, int cap, const float* d_pose,
                                           const uint8_t* d_kf_bad, const int* d_obs_ptr,
                                           const orbm_observation* d_obs, const orbm_observation* d_ref, int np,
                                           int max_obs, const orbm_pose_params* params, orbm_map_point* d_pts,
                                           uint8_t* d_pdesc, int* d_best, void* stream);

/* Host arrays, on HIP device `device`; pts and pdesc are updated in place.  max_obs is worked out from obs_ptr:
 * ORBX_EINVAL when a list is longer than ORBM_MAX_OBSERVATIONS or obs_ptr does not ascend from >= 0.
 * Synchronous. */
orbx_status orbm_refresh_map_points(int device, int what, const orbx_keypoint* kps, const uint8_t* desc,
                                    const int* counts, int nkf, int cap, const float* pose, const uint8_t* kf_bad,
                                    const int* obs_ptr, const orbm_observation* obs, const orbm_observation* ref,
                                    int np, const orbm_pose_params* params, orbm_map_point* pts, uint8_t* pdesc,
                                    int* best);

/* ---- Sim3Solver: the RANSAC of LoopClosing::ComputeSim3 between SearchByBoW and SearchBySim3 ----
 * src/Sim3Solver.cc (constructor :37-112, SetRansacParameters :114-138, iterate :140-207, ComputeSim3 :226-337,
 * CheckInliers :340-364, Project / FromCameraToImage :382-423), as src/LoopClosing.cc:274-323 drives it.  Horn's
 * closed-form 3-point solve (cv::eigen's Jacobi on the 4x4 N, cv::Rodrigues) and the projection test of every
 * hypothesis, batched over solvers and iterations.  The arithmetic order is fixed in DESIGN.md §3 "Sim3 solver
 * arithmetic"; parity with a real OpenCV is unpinned.  OptimizeSim3 follows below (orbm_optimize_sim3_device).
 *
 * orbm_sim3_setup_device = the constructor and SetRansacParameters, one solver per pair p: KF1 = d_pair_a[p]
 * (mpCurrentKF), KF2 = d_pair_b[p].  KeyFrame table: the layout of orbm_search_by_sim3_device (d_kps = mvKeysUn,
 * d_counts, cap, d_pose[f * 12] = row-major 3x4 Tcw) plus d_kf_mp[f * cap + i] = GetMapPointMatches()[i] as an index
 * into d_pts, -1 none.  MapPoint table: d_pts (x, y, z and flags bit 0 = !isBad() are read), nmp, and the
 * observation lists d_obs[d_obs_ptr[m] .. d_obs_ptr[m + 1]) with d_obs_erased (NULL = none erased) as in
 * orbm_map_point_culling_device.  d_match12[p * match_stride + i1] = idx2 or -1 as orbm_bow_search_device
 * (ORBM_BOW_KF_KF) leaves it, match_stride >= cap: vpMatched12[i1] = d_kf_mp[b * cap + idx2].  Both cameras share
 * one orbm_pose_params; fx, fy, cx, cy, nlevels and scale[] are read (mvLevelSigma2[o] = scale[o] * scale[o]).
 * A pair survives as the reference has it: both MapPoints present and not bad, and GetIndexInKeyFrame -- the idx
 * of the point's live observation whose kf is the KeyFrame -- >= 0 on both sides; the keypoints are those at
 * indexKF1 / indexKF2, not at i1 / idx2.  The stored error bounds are (float)(size_t)(9.210 * sigma2): mvnMaxError
 * is a vector<size_t>.  The survivors are kept in i1 order in d_work.
 * d_maxits[n], n <= cap, is mRansacMaxIts for N = n: orbm_sim3_ransac_iterations(n, probability, min_inliers,
 * max_iterations), filled by the caller once per parameter set.  Outputs: d_n[p] = N, d_iterations[p] =
 * d_best_inliers[p] = 0 (mnIterations, mnBestInliers), d_status[p] = 0 or ORBM_SIM3_INVALID.  Invalid: a KeyFrame
 * slot outside [0, nkf), a count outside [0, cap], a d_match12 entry outside [-1, count of KF2), a d_kf_mp entry
 * outside [-1, nmp), a descending d_obs_ptr, the observation of a survivor with idx outside its KeyFrame's count,
 * or its keypoint's octave outside [0, nlevels).  Of an invalid solver only d_status[p] is written, and iterate
 * gives it no result.
 *
 * orbm_sim3_iterate_device = iterate(nit, bNoMore, vbInliers, nInliers) of every solver.  Iterations k < nit are
 * evaluated as independent hypotheses and the reference's sequential rule is then applied: with best_k =
 * max(d_best_inliers, inliers of the iterations before k) the call returns at the first k whose inliers are >=
 * best_k and > min_inliers; it stops when d_iterations + k + 1 reaches mRansacMaxIts.  Iteration k of solver p
 * draws its three points from d_rand[d_rand_off[p] + 3k .. + 2], raw rand() values in [0, 2^31 - 1], through
 * DUtils::Random::RandomInt and the swap-with-back removal of :163-177.  fix_scale = mbFixScale.
 * Outputs per solver: d_sim3[p * 13] = s12, R12 (row-major), t12 of the returned hypothesis, all 0 without one
 * (orbm_search_by_sim3_device: s12 not > 0 matches nothing); d_inliers12[p * cap + i1] = vbInliers (and the
 * d_already1 of orbm_search_by_sim3_device); d_already2[p * cap + i2] = vbAlreadyMatched2 as SearchBySim3
 * :1200-1210 derives it from the inliers, through GetIndexInKeyFrame(pKF2); d_ninliers[p] = nInliers; d_nomore[p]
 * = bNoMore; d_used[p] = the iterations this call consumed (so the draws of the next call start 3 * d_used
 * further).  d_iterations / d_best_inliers are read and updated.  N < min_inliers is bNoMore with nothing else
 * done; a negative d_iterations (a state the calls never leave) is bNoMore without a result too.  nsolvers and nit
 * are at most 65535 each (orbm_sim3_workspace_bytes returns 0 beyond).  nit in [1, max_iters_per_call of the
 * workspace]; min_inliers >= 3 (the reference's sampling is undefined
 * below it).  d_work of orbm_sim3_workspace_bytes(nsolvers, cap, max_iters_per_call) bytes, 16-byte aligned, keeps
 * the solvers between the calls.  ORBX_EINVAL for a null or misaligned argument, cap outside [1,
 * ORBM_MAX_FEATURES], nsolvers or nit above 65535, min_inliers < 3 or a workspace too small.  Both calls allocate nothing and are asynchronous
 * on `stream`. */
enum { ORBM_SIM3_INVALID = 1 };   /* d_status bits */

size_t orbm_sim3_workspace_bytes(int nsolvers, int cap, int max_iters_per_call);

/* mRansacMaxIts of SetRansacParameters for N = n (:125-135), the reference's expression on the host's libm: 1 when
 * min_inliers == n, else max(1, min(ceil(log(1 - p) / log(1 - pow(eps, 3))), max_iterations)) with float eps =
 * (float)min_inliers / n.  A quotient that is not a number or outside int converts as x86 does (INT_MIN). */
int orbm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations);

orbx_status orbm_sim3_setup_device(const orbx_keypoint* d_kps, const int* d_counts, int nkf, int cap,
                                   const float* d_pose, const int* d_kf_mp, const orbm_map_point* d_pts, int nmp,
                                   const int* d_obs_ptr, const orbm_observation* d_obs, const uint8_t* d_obs_erased,
                                   const int* d_pair_a, const int* d_pair_b, int nsolvers, const int* d_match12,
                                   int match_stride, const orbm_pose_params* params, const int* d_maxits,
                                   void* d_work, size_t work_bytes, int* d_n, int* d_iterations, int* d_best_inliers,
                                   int* d_status, void* stream);

orbx_status orbm_sim3_iterate_device(void* d_work, size_t work_bytes, int nsolvers, int cap,
                                     const orbm_pose_params* params, int fix_scale, int min_inliers, int nit,
                                     const int* d_rand, const int* d_rand_off, int* d_iterations, int* d_best_inliers,
                                     float* d_sim3, uint8_t* d_inliers12, uint8_t* d_already2, int* d_ninliers,
                                     int* d_nomore, int* d_used, void* stream);

/* One pair on host arrays, on HIP device `device`; synchronous: the constructor, SetRansacParameters(probability,
 * min_inliers, max_iterations) and one iterate(nit) that starts from *iterations and *best_inliers (0, 0 for a new
 * solver; both are updated).  KeyFrame 1: kps1, kf_mp1, n1, T1w (12 floats); likewise KeyFrame 2; they count as
 * slots 0 and 1 in the observations.  match12: n1 ints; rand: 3 * nit ints.  Outputs: *n, sim3 (13 floats),
 * inliers12 (n1 bytes), already2 (n2 bytes), *ninliers, *nomore, *used, *status; of an invalid solver only *status
 * is written. */
orbx_status orbm_sim3_solve(int device, const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                            const orbx_keypoint* kps2, const int* kf_mp2, int n2, const float* T2w,
                            const orbm_map_point* pts, int nmp, const int* obs_ptr, const orbm_observation* obs,
                            const uint8_t* obs_erased, const int* match12, const orbm_pose_params* params,
                            int fix_scale, double probability, int min_inliers, int max_iterations, int nit,
                            const int* rand, int* iterations, int* best_inliers, int* n, float* sim3,
                            uint8_t* inliers12, uint8_t* already2, int* ninliers, int* nomore, int* used, int* status);

/* Test hooks, not part of the interface a caller builds on (they may change or go without notice).
 * orbm_sim3_solve_host: the kernels' own code compiled for the CPU and run by one lane, the arguments and results of
 * orbm_sim3_solve without a device; tests/test_sim3_solver.py compares it with its restatement bit for bit. */
orbx_status orbm_sim3_solve_host(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                                 const orbx_keypoint* kps2, const int* kf_mp2, int n2, const float* T2w,
                                 const orbm_map_point* pts, int nmp, const int* obs_ptr, const orbm_observation* obs,
                                 const uint8_t* obs_erased, const int* match12, const orbm_pose_params* params,
                                 int fix_scale, double probability, int min_inliers, int max_iterations, int nit,
                                 const int* rand, int* iterations, int* best_inliers, int* n, float* sim3,
                                 uint8_t* inliers12, uint8_t* already2, int* ninliers, int* nomore, int* used,
                                 int* status);

/* Test hook: atan2 as the Sim3 solver evaluates it (csrc/orbx_math.hpp fixed_atan2). */
double orbx_fixed_atan2(double y, double x);

/* Test hook: the three correspondences iteration draws r[0..2] select among n (RandomInt and the removal). */
void orbx_sim3_triplet(int n, const int* r, int* out3);

/* ---- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) ----
 * src/Optimizer.cc:1046-1241, which LoopClosing::ComputeSim3 calls between SearchBySim3 and SearchByProjection(pKF,
 * Scw, ...) (src/LoopClosing.cc:325-335): one free 7-DoF Sim3 vertex, per correspondence the two projection edges
 * EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ with fixed points and Huber kernels, g2o's Levenberg on a dense
 * 7x7 system with the numeric Jacobian of base_binary_edge.hpp, optimize(5), the first inlier check, optimize(10 or
 * 5), the second check.  One workgroup per pair; the arithmetic order is fixed in DESIGN.md §3 "Sim3 optimisation
 * arithmetic"; parity with a real g2o / Eigen build is unpinned.
 *
 * orbm_optimize_sim3_device.  KeyFrame and MapPoint tables, pairs and params: those of orbm_sim3_setup_device (of
 * params fx, fy, cx, cy, nlevels and inv_sigma2[] are read; both cameras share them).  d_sim3_in[p * 13] = s12, R12,
 * t12 as orbm_sim3_iterate_device writes them: the initial estimate is Sim3(toMatrix3d(R), toVector3d(t), (double)s).
 * d_matches1[p * match_stride + i1] (in / out) = vpMatches1[i1] as an index into d_pts, -1 none, match_stride >= cap.
 * th2 and fix_scale: the reference passes 10 and mbFixScale.
 * Feature i1 of KF1 makes a correspondence when d_matches1 >= 0, pMP1 = d_kf_mp[a * cap + i1] is present and not
 * bad, pMP2 is not bad and i2 = pMP2->GetIndexInKeyFrame(pKF2) >= 0 (the live observation, as orbm_sim3_setup_device
 * finds it); any other entry of d_matches1 is left as it is.  An entry is set to -1 where either edge's chi2 exceeds
 * th2 after a round.
 * Outputs: d_nin[p] the return value (0 where fewer than 10 correspondences survive the first check); d_sim3_out[p *
 * 8] doubles qx, qy, qz, qw, tx, ty, tz, s, the g2o::Sim3 itself; d_sim3f_out[p * 13] (may be NULL) floats s, R, t in
 * the format of d_sim3_in; d_scw[p * 12] (may be NULL) the top three rows of Converter::toCvMat(gScm * gSmw) with
 * gSmw = Sim3(R2w, t2w, 1.0) (src/LoopClosing.cc:333-335), the pose ORBM_PROJ_SIM3 reads; d_trace[p] (may be NULL);
 * d_status[p] 0 or ORBM_OPT_SIM3_INVALID.  The three Sim3 outputs are written only where the reference reaches
 * :1237 (trace rounds == 2); they keep their bits otherwise.
 * Invalid: what orbm_sim3_setup_device lists (slots, counts, d_kf_mp, a descending d_obs_ptr, an observation idx, an
 * octave), a d_matches1 entry outside [-1, nmp) and an s12 that is not > 0.  Of an invalid pair only d_status[p] is
 * written.  ORBX_EINVAL for a null or misaligned argument (d_sim3_out: 8 bytes), cap outside [1, ORBM_MAX_FEATURES],
 * match_stride < cap or npairs above 65535.  Allocates nothing; asynchronous on `stream`. */
enum { ORBM_OPT_SIM3_INVALID = 1 };   /* d_status bits */

typedef struct {
    int32_t iters[2];      /* SparseOptimizer::optimize's iterations of the two rounds */
    int32_t rejected[2];   /* Levenberg trials rejected and popped */
    int32_t nbad;          /* nBad of the first check */
    int32_t ncorr;         /* nCorrespondences */
    int32_t rounds;        /* rounds run: 0 (no correspondence), 1 (fewer than 10 left) or 2 */
} orbm_opt_sim3_trace;

orbx_status orbm_optimize_sim3_device(const orbx_keypoint* d_kps, const int* d_counts, int nkf, int cap,
                                      const float* d_pose, const int* d_kf_mp, const orbm_map_point* d_pts, int nmp,
                                      const int* d_obs_ptr, const orbm_observation* d_obs,
                                      const uint8_t* d_obs_erased, const int* d_pair_a, const int* d_pair_b,
                                      int npairs, const float* d_sim3_in, int* d_matches1, int match_stride, float th2,
                                      int fix_scale, const orbm_pose_params* params, double* d_sim3_out,
                                      float* d_sim3f_out, float* d_scw, int* d_nin, orbm_opt_sim3_trace* d_trace,
                                      int* d_status, void* stream);

/* vpMapPointMatches as src/LoopClosing.cc:313-318 builds it and SearchBySim3 (:323) extends it, on the device:
 * d_matches1[p * match_stride + i1] = d_inliers12[p * cap + i1] ? d_kf_mp[b * cap + d_bow_match12[p * bow_stride +
 * i1]] : d_sbs_match12[p * cap + i1] >= 0 ? d_kf_mp[b * cap + d_sbs_match12[p * cap + i1]] : -1, with d_inliers12 of
 * orbm_sim3_iterate_device, d_bow_match12 the d_match12 given to orbm_sim3_setup_device and d_sbs_match12 the
 * d_match12 of orbm_search_by_sim3_device.  Every i1 < cap is written: -1 at and past KF1's count, for a feature
 * index outside KF2's count and for a pair whose slots are outside [0, nkf).  Asynchronous on `stream`. */
orbx_status orbm_sim3_gather_matches_device(const int* d_kf_mp, const int* d_counts, int nkf, int cap,
                                            const int* d_pair_a, const int* d_pair_b, int npairs,
                                            const uint8_t* d_inliers12, const int* d_bow_match12, int bow_stride,
                                            const int* d_sbs_match12, int* d_matches1, int match_stride, void* stream);

/* One pair on host arrays, on HIP device `device`; synchronous.  KeyFrame 1: kps1, kf_mp1, n1, T1w (12 floats);
 * KeyFrame 2: kps2, n2, T2w; they count as slots 0 and 1 in the observations.  sim3_in: 13 floats; matches1: n1 ints,
 * updated in place; sim3_out 8 doubles, sim3f_out 13 floats and scw 12 floats (either may be NULL), written only
 * where the reference reaches :1237; trace may be NULL.  Of an invalid pair only *status is written. */
orbx_status orbm_optimize_sim3(int device, const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                               const orbx_keypoint* kps2, int n2, const float* T2w, const orbm_map_point* pts, int nmp,
                               const int* obs_ptr, const orbm_observation* obs, const uint8_t* obs_erased,
                               const float* sim3_in, int* matches1, float th2, int fix_scale,
                               const orbm_pose_params* params, double* sim3_out, float* sim3f_out, float* scw,
                               int* nin, orbm_opt_sim3_trace* trace, int* status);

/* Test hooks, not part of the interface a caller builds on (they may change or go without notice).
 * orbm_optimize_sim3_host: the kernel's own code compiled for the CPU and run by one lane, the arguments and results
 * of orbm_optimize_sim3 without a device; tests/test_optimize_sim3.py compares it with its restatement bit for bit. */
orbx_status orbm_optimize_sim3_host(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                                    const orbx_keypoint* kps2, int n2, const float* T2w, const orbm_map_point* pts,
                                    int nmp, const int* obs_ptr, const orbm_observation* obs,
                                    const uint8_t* obs_erased, const float* sim3_in, int* matches1, float th2,
                                    int fix_scale, const orbm_pose_params* params, double* sim3_out, float* sim3f_out,
                                    float* scw, int* nin, orbm_opt_sim3_trace* trace, int* status);

/* Test hook: exp as the Sim3 optimiser evaluates it (csrc/orbx_math.hpp fixed_exp). */
double orbx_fixed_exp(double x);

/* ---- Initializer: the two-view initialisation of Tracking::MonocularInitialization ----
 * src/Initializer.cc: Initialize (:45-159), FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography,
 * CheckFundamental, ReconstructF, ReconstructH, DecomposeE, CheckRT, Triangulate and Normalize, statement by
 * statement, batched over frame pairs: the call that follows SearchForInitialization in src/Tracking.cc.  The
 * arithmetic order is fixed in DESIGN.md §3 "Initializer arithmetic"; parity with a real OpenCV is unpinned.
 *
 * orbm_initialize_device.  Frame table: d_kps[f * cap + i] = mvKeysUn (x and y are read), d_counts[f], nframes.
 * Pair p: frame 1 (the reference frame) = d_pair_a[p], frame 2 (the current frame) = d_pair_b[p].
 * d_matches12[p * match_stride + i] = vMatches12[i] as orbm_search_init_batch_device leaves it, -1 none, match_stride
 * >= cap; never written.  d_draws[p * draws_stride + 8 * it + j] = the raw rand() value (0 .. 2^31 - 1) draw j of
 * iteration `it` consumes through DUtils::Random::RandomInt, draws_stride >= 8 * max_iterations: SeedRandOnce(0)
 * seeds once per process and every caller shares the generator, so the values are the caller's.  params: fx, fy,
 * cx, cy are read (mK).  sigma and max_iterations are the constructor's (1.0, 200); minParallax = 1.0 and
 * minTriangulated = 50 as Initialize passes them.
 * Outputs per pair, arrays of npairs entries of the size given:
 *   status          0, or ORBM_INIT_INVALID / ORBM_INIT_NO_MODEL / ORBM_INIT_FAILED
 *   model           0 none, 1 the homography (RH > 0.40), 2 the fundamental matrix
 *   reason          for ORBM_INIT_FAILED the `return false` taken (orbm_init_reason), else 0
 *   scores[2]       SH, SF
 *   H21[9], F21[9]  the best-scoring matrices, zeros where no hypothesis scored above 0
 *   inliersH[cap], inliersF[cap]   vbMatchesInliersH / F as bytes indexed by the frame-1 keypoint, 0 where unmatched
 *   R21[9], t21[3]  zeros unless status is 0
 *   p3d[cap * 3], triangulated[cap]   vP3D and vbTriangulated, indexed by the frame-1 keypoint; zeros unless
 *                   status is 0.  vP3D is written wherever the reference writes it (:1252), vbTriangulated only
 *                   where cosParallax < 0.99998
 *   ngood[8], parallax[8]   nGood and parallax of every CheckRT in the reference's order (ReconstructF fills 4)
 *   nmatches_left   the matches that remain after MonocularInitialization's pruning loop; N unless status is 0
 *   matches_out[match_stride]   with ORBM_INIT_PRUNE_MATCHES: the row of d_matches12 with that loop applied
 *                   ("if(mvIniMatches[i]>=0 && !vbTriangulated[i]) mvIniMatches[i]=-1" after a successful
 *                   Initialize), a plain copy otherwise; may be NULL without the flag
 * ORBM_INIT_INVALID, and nothing else written: a pair index outside [0, nframes), a count outside [0, cap], a match
 * outside [-1, count of frame 2), fewer than 8 matches (RandomInt(0, size - 1) is undefined there), max_iterations
 * outside [1, 4096] (orbm_init_workspace_bytes returns 0 there).  ORBM_INIT_NO_MODEL: no hypothesis scored above 0,
 * where the reference reads an empty cv::Mat.
 * d_work of orbm_init_workspace_bytes(npairs, cap, max_iterations) bytes, 16-byte aligned; a workspace sized for more
 * iterations serves fewer.  ORBX_EINVAL, before any launch, for a null or misaligned argument, cap outside [1,
 * ORBM_MAX_FEATURES], npairs above 65535, sigma <= 0, an unknown flag or a workspace too small.  Allocates nothing,
 * asynchronous on `stream`. */
enum { ORBM_INIT_INVALID = 1, ORBM_INIT_NO_MODEL = 2, ORBM_INIT_FAILED = 4 };   /* status bits */
enum { ORBM_INIT_PRUNE_MATCHES = 1 };                                          /* flags */
typedef enum {
    ORBM_INIT_REASON_NONE = 0,
    ORBM_INIT_F_AMBIGUOUS = 1,   /* :739  maxGood < nMinGood || nsimilar > 1 */
    ORBM_INIT_F_PARALLAX = 2,    /* :745-791  the winning candidate's parallax is not above minParallax */
    ORBM_INIT_H_SINGULAR = 3,    /* :845  d1/d2 < 1.00001 || d2/d3 < 1.00001 */
    ORBM_INIT_H_TEST = 4         /* :987  the final test fails */
} orbm_init_reason;

typedef struct {
    int32_t *status, *model, *reason;
    float *scores, *H21, *F21;
    uint8_t *inliersH, *inliersF;
    float *R21, *t21, *p3d;
    uint8_t* triangulated;
    int32_t* ngood;
    float* parallax;
    int32_t* nmatches_left;
    int32_t* matches_out;
} orbm_init_out;

/* A pure size planner: 0 for what orbm_initialize_device does not accept. */
size_t orbm_init_workspace_bytes(int npairs, int cap, int max_iterations);

orbx_status orbm_initialize_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                   const int* d_pair_a, const int* d_pair_b, int npairs, const int* d_matches12,
                                   int match_stride, const int* d_draws, int draws_stride,
                                   const orbm_pose_params* params, float sigma, int max_iterations, int flags,
                                   void* d_work, size_t work_bytes, const orbm_init_out* out, void* stream);

/* One pair on host arrays, on HIP device `device`; synchronous.  kps1 (n1), kps2 (n2), matches12 (n1), draws (8 *
 * max_iterations); `out` points at host arrays of one pair with n1 in the place of cap and of match_stride.  Of an
 * invalid pair only *out->status is written. */
orbx_status orbm_initialize(int device, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                            const int* matches12, const int* draws, const orbm_pose_params* params, float sigma,
                            int max_iterations, int flags, const orbm_init_out* out);

/* Test hooks, not part of the interface a caller builds on.  orbm_initialize_host: the kernels' own code compiled
 * for the CPU and run by one lane, the arguments and results of orbm_initialize without a device;
 * tests/test_initializer.py compares it with its restatement bit for bit. */
orbx_status orbm_initialize_host(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                                 const int* matches12, const int* draws, const orbm_pose_params* params, float sigma,
                                 int max_iterations, int flags, const orbm_init_out* out);

/* mvSets (:88-120) for n matches: sets[8 * it + j] from draws[8 * it + j], RandomInt and the swap-with-back removal.
 * n >= 8. */
void orbx_init_sets(int n, const int* draws, int iterations, int* sets);

/* Test hook: acosf as CheckRT's parallax evaluates it (csrc/orbx_math.hpp fixed_acosf). */
float orbx_fixed_acosf(float x);

/* ---- PnPsolver: the EPnP RANSAC of Tracking::Relocalization between SearchByBoW(KF, F) and PoseOptimization ----
 * src/PnPsolver.cc (constructor :67-110, SetRansacParameters :121-157, iterate :165-258, Refine :260-305,
 * CheckInliers :308-339, compute_pose and everything under it :375-950), as src/Tracking.cc:1393-1554 drives it,
 * batched over solvers: one solver is one (frame, candidate KeyFrame) pair.  Every iteration of a call is evaluated
 * as an independent hypothesis, then the reference's sequential acceptance rule is applied.  The arithmetic order
 * (EPnP in double, the OpenCV calls as OpenCV 3.x's generic path) is fixed in DESIGN.md §3 "PnP solver arithmetic";
 * parity with a real OpenCV is unpinned.  The nmatches < 15 discard, the round-robin over the candidates, sFound and
 * the two follow-up SearchByProjection calls, the nGood thresholds and the copy of the chosen solver's rows into the
 * frame stay with the caller.
 *
 * orbm_pnp_setup_device = the constructor and SetRansacParameters, one solver per pair p: frame d_frame_of[p],
 * KeyFrame d_kf_of[p].  Frame table: d_kps (mvKeysUn; x, y and octave are read) at f * cap, d_counts[f] features,
 * nframes.  KeyFrame table: d_kf_mp[kf * cap + i] = GetMapPointMatches()[i] as an index into d_pts, -1 none, nkf rows.
 * d_match[p * match_stride + iF] = the KeyFrame feature orbm_bow_search_device (ORBM_BOW_KF_F) assigned to frame
 * feature iF, -1 none, match_stride >= cap: vpMapPointMatches[iF] = d_kf_mp[kf * cap + d_match[..]].  An entry survives
 * if the MapPoint index is >= 0 and flags bit 0 (!isBad()) of the orbm_map_point is set; the survivors are kept in iF
 * order in d_work with mvP2D = the keypoint's x, y, mvSigma2 = scale[octave]^2, mvP3Dw = the point's x, y, z and
 * mvKeyPointIndices = iF.  Of params fx, fy, cx, cy (fu, fv, uc, vc), nlevels and scale[] are read.  mvMaxError =
 * sigma2 * th2 in float.  d_min_inliers[n] and d_maxits[n], n <= cap, are the adjusted mRansacMinInliers and
 * mRansacMaxIts for N = n (orbm_pnp_ransac_parameters), filled by the caller once per parameter set: only the last
 * SetRansacParameters call counts, as every field is overwritten.  max_iterations is the maxIterations of that call.
 * Outputs: d_n[p] = N, d_iterations[p] = d_best_inliers[p] = 0 (mnIterations, mnBestInliers), d_status[p] = 0 or
 * ORBM_PNP_INVALID.  Invalid: a frame or KeyFrame slot out of range, a count outside [0, cap], a d_match entry outside
 * [-1, cap), a d_kf_mp entry outside [-1, nmp), the octave of a survivor outside [0, nlevels), or table entries the
 * calls cannot run with (d_min_inliers[N] < 4, d_maxits[N] outside [1, max_iterations]).  Of an invalid solver only
 * d_status[p] is written, and iterate gives it no result.
 *
 * orbm_pnp_iterate_device = iterate(nit, bNoMore, vbInliers, nInliers) of every solver.  The reference's loop is
 * while(mnIterations < mRansacMaxIts || nCurrentIterations < nIterations), an OR: a call consumes max(nit,
 * mRansacMaxIts - mnIterations) iterations unless it returns through Refine(), a call that does not return through
 * Refine() always ends with bNoMore, and a solver called again at or past mRansacMaxIts runs exactly nit more.
 * Iteration k of solver p draws its four points from d_rand[d_rand_off[p] + 4k .. + 3], raw rand() values in [0,
 * 2^31 - 1], through DUtils::Random::RandomInt and the swap-with-back removal; d_rand holds nrand values and a solver
 * needs 4 * max(nit, max_iterations) of them from its offset on (an iteration whose draws lie outside d_rand counts
 * as one without inliers).  An iteration with mnInliersi >= mRansacMinInliers replaces the best when strictly greater
 * and then calls Refine() on the best set: Refine() succeeds on more than mRansacMinInliers inliers (strict), and the
 * call returns mRefinedTcw, mvbRefinedInliers and mnRefinedInliers.  On exhaustion the call returns mBestTcw
 * (unrefined) and the best mask if mnBestInliers >= mRansacMinInliers, else no pose.  Refine() is a function of the
 * best set alone: it is evaluated where the best changes, and its outcome is kept in the solver between the calls, so
 * a solver that returned through Refine() returns again at its next qualifying iteration.
 * Outputs per solver: d_tcw[p * 12] = row-major 3x4 Tcw (the CV_64F -> CV_32F conversion of R, t), all 0 without a
 * pose: the d_pose_in of orbm_pose_optimization_device at stride 12; d_has_pose[p]; d_inliers[p * cap + iF] =
 * vbInliers; d_ninliers[p] = nInliers; d_nomore[p] = bNoMore; d_used[p] = the iterations this call consumed (the draws
 * of the next call start 4 * d_used further); d_frame_mp_out[p * cap + iF] = the MapPoint index of an inlier, else -1
 * (src/Tracking.cc:1481-1490, the d_frame_mp of orbm_pose_optimization_device).  d_iterations / d_best_inliers are
 * read and updated.  N < mRansacMinInliers is bNoMore with nothing else done; a negative d_iterations is bNoMore
 * without a result too.
 * One place the reference is undefined: qr_solve returns early on eta == 0 and leaves X untouched, an uninitialised
 * stack array on the first Gauss-Newton step.  Here x is zero at the start of each gauss_newton and keeps its
 * previous content after an early return; the static A1 / A2 are locals.
 * d_work of orbm_pnp_workspace_bytes(nsolvers, cap, max_iters_per_call) bytes, 16-byte aligned, keeps the solvers
 * between the calls; max_iters_per_call >= max(nit, max_iterations) of every iterate call.  ORBX_EINVAL before any
 * launch for a null or misaligned argument, cap outside [1, ORBM_MAX_FEATURES], nsolvers, nit or max_iterations above
 * 65535, min_set != 4 or a workspace too small.  Both calls allocate nothing and are asynchronous on `stream`. */
enum { ORBM_PNP_INVALID = 1 };   /* d_status bits */

size_t orbm_pnp_workspace_bytes(int nsolvers, int cap, int max_iters_per_call);

/* SetRansacParameters for N = n (:129-152), the reference's expressions on the host's libm: int nMinInliers = N *
 * (float)epsilon, raised to min_inliers and to min_set; float epsilon raised to (float)nMinInliers / N; 1 iteration
 * when nMinInliers == N, else ceil(log(1 - p) / log(1 - pow(eps, 3))); max(1, min(.., max_iterations)).  A value that
 * is not a number or outside int converts as x86 does (INT_MIN).  Tracking passes (0.99, 10, 300, 4, 0.5, 5.991). */
void orbm_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set,
                                float epsilon, int* out_min_inliers, int* out_max_iterations);

orbx_status orbm_pnp_setup_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                  const int* d_kf_mp, int nkf, const orbm_map_point* d_pts, int nmp,
                                  const int* d_frame_of, const int* d_kf_of, int nsolvers, const int* d_match,
                                  int match_stride, const orbm_pose_params* params, float th2,
                                  const int* d_min_inliers, const int* d_maxits, int max_iterations, void* d_work,
                                  size_t work_bytes, int* d_n, int* d_iterations, int* d_best_inliers, int* d_status,
                                  void* stream);

orbx_status orbm_pnp_iterate_device(void* d_work, size_t work_bytes, int nsolvers, int cap,
                                    const orbm_pose_params* params, int min_set, int max_iterations, int nit,
                                    const int* d_rand, int nrand, const int* d_rand_off, int* d_iterations,
                                    int* d_best_inliers, float* d_tcw, int* d_has_pose, uint8_t* d_inliers,
                                    int* d_ninliers, int* d_nomore, int* d_used, int* d_frame_mp_out, void* stream);

/* One solver on host arrays, on HIP device `device`; synchronous: the constructor, SetRansacParameters(probability,
 * min_inliers, max_iterations, min_set, epsilon, th2) and one iterate(nit).  State in and out: *iterations and
 * *best_inliers (0, 0 for a new solver) and `state`, orbm_pnp_state_bytes(max(n, nk)) bytes, 8-byte aligned (the best
 * and the refined pose and masks and Refine()'s outcome; not read when *iterations is 0, always written).  kps: the
 * frame's n mvKeysUn; kf_mp: the KeyFrame's nk MapPoint indices; match: n ints; rand: 4 * max(nit, max_iterations)
 * ints.  Outputs: *n_out, tcw (12 floats), *has_pose, inliers (n bytes), *ninliers, *nomore, *used, frame_mp_out (n
 * ints), *status; of an invalid solver only *status is written. */
size_t orbm_pnp_state_bytes(int cap);

orbx_status orbm_pnp_solve(int device, const orbx_keypoint* kps, int n, const int* kf_mp, int nk,
                           const orbm_map_point* pts, int nmp, const int* match, const orbm_pose_params* params,
                           float th2, double probability, int min_inliers, int max_iterations, int min_set,
                           float epsilon, int nit, const int* rand, int* iterations, int* best_inliers, void* state,
                           int* n_out, float* tcw, int* has_pose, uint8_t* inliers, int* ninliers, int* nomore,
                           int* used, int* frame_mp_out, int* status);

/* Test hooks, not part of the interface a caller builds on (they may change or go without notice).
 * orbm_pnp_solve_host: the kernels' own code compiled for the CPU and run by one lane, the arguments and results of
 * orbm_pnp_solve without a device; tests/test_pnp_solver.py compares it with its restatement bit for bit.  trace (may
 * be NULL with trace_cap 0) receives, for the iterations consumed and then for the Refine() calls, what each
 * compute_pose met: bit a (a = 1, 2, 3) of a field is find_betas_approx_a's branch. */
typedef struct {
    int32_t refine;        /* 0 an iteration, 1 a Refine() */
    int32_t N;             /* the approximation chosen (1, 2, 3) */
    int32_t b_neg;         /* b[0] < 0 */
    int32_t b1_neg;        /* b[1] < 0 (approx 2 and 3) */
    int32_t sign_flip;     /* solve_for_sign flipped */
    int32_t det_flip;      /* det < 0 in estimate_R_and_t */
    int32_t qr_singular;   /* qr_solve returned on eta == 0 */
    int32_t inliers;       /* mnInliersi of an iteration */
} orbm_pnp_trace;

orbx_status orbm_pnp_solve_host(const orbx_keypoint* kps, int n, const int* kf_mp, int nk, const orbm_map_point* pts,
                                int nmp, const int* match, const orbm_pose_params* params, float th2,
                                double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                int nit, const int* rand, int* iterations, int* best_inliers, void* state,
                                int* n_out, float* tcw, int* has_pose, uint8_t* inliers, int* ninliers, int* nomore,
                                int* used, int* frame_mp_out, int* status, orbm_pnp_trace* trace, int trace_cap,
                                int* ntrace);

/* Test hooks: the four correspondences iteration draws r[0..3] select among n >= 4 (RandomInt and the removal);
 * qr_solve of a 6x4 system (A24 and b6 are overwritten; returns 1, or 0 where the reference returns early on eta == 0
 * and x4 keeps its content); cvSVD(A, D, Ut, 0, CV_SVD_MODIFY_A | CV_SVD_U_T) of a 12x12. */
void orbx_pnp_quad(int n, const int* r, int* out4);
int orbx_pnp_qr_solve(double* A24, double* b6, double* x4);
void orbx_pnp_svd12(const double* A144, double* ut144, double* w12);

/* ---- New MapPoints: the match loop of LocalMapping::CreateNewMapPoints ----
 * src/LocalMapping.cc:284-450, between SearchForTriangulation (orbm_bow_search_device, ORBM_TRIANGULATION) and the
 * MapPoint refresh above.  For every vMatchedPairs entry: the parallax of the two rays, a 4x4 cv::SVD triangulation
 * or KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631), the depth signs, the chi-square reprojection error (5.991
 * mono, 7.8 stereo) and the scale consistency test; what passes becomes a MapPoint.  ComputeF12, the baseline test
 * and ComputeSceneMedianDepth (:244-264) stay with the caller, who fills orbm_triang_params and chooses the pairs.
 *
 * KeyFrame table: the layout of orbm_search_by_sim3_device / orbm_refresh_map_points_device (d_kps = mvKeysUn,
 * d_counts, cap, d_pose[f * 12] = row-major 3x4 Tcw) plus d_kps_raw = mvKeys (NULL = d_kps; UnprojectStereo reads
 * mvKeys, src/KeyFrame.cc:620) and d_uright / d_depth = mvuRight / mvDepth (both NULL = monocular, all -1).  Pair p:
 * KF1 = d_pair_a[p] (mpCurrentKeyFrame), KF2 = d_pair_b[p] (the neighbour), d_match[p * match_stride + idx1] = idx2
 * as orbm_bow_search_device leaves it, match_stride >= cap.  Both KeyFrames share one orbm_pose_params; of it only
 * fx, fy, cx, cy, bf, b, nlevels and scale[] are read: invfx = 1.0f / fx, mvLevelSigma2[o] = scale[o] * scale[o],
 * ratioFactor = 1.5f * scale[1].  With shared intrinsics the reference's use of mpCurrentKeyFrame->mbf for
 * KeyFrame 2 (:406) makes no difference.
 *
 * d_status[p * match_stride + idx1], idx1 < cap, one orbm_triang_status each.  A pair whose KeyFrame slot is outside
 * [0, nkf) gets ORBM_TRI_INVALID in all its cap entries.  Otherwise the range checks come before any indexed read:
 * idx2 outside [0, min(d_counts[kf2], cap)), a keypoint octave outside [0, nlevels), or a stereo keypoint
 * (uright >= 0) whose depth is not > 0 (the reference would dereference an empty Mat) give ORBM_TRI_INVALID, and
 * nothing but the status is written for the entry.  d_x3d[(p * match_stride + idx1) * 3 ..] is written for created
 * points only; every other entry keeps its bits.
 *
 * Compacted outputs: pair p's created points at d_new_*[p * match_stride + k], k < d_nnew[p], in ascending idx1 --
 * the order of vMatchedIndices and so of mlpRecentAddedMapPoints.  d_new_pts[k]: x, y, z, flags = 3 (not bad,
 * Observations() > 0), all else 0.  d_new_obs[2k], [2k + 1]: (kf1, idx1) and (kf2, idx2), the KeyFrame with the
 * smaller d_kf_rank first (d_kf_rank[f] = the position of KeyFrame f in the caller's std::map<KeyFrame*, size_t>
 * order; NULL = slot order).  With two observations both medians of ComputeDistinctiveDescriptors are 0 and it keeps
 * the first row, so this order decides the descriptor.  d_new_ref[k] = (kf1, idx1): mpRefKF is the current
 * KeyFrame.  d_new_idx1[k] = idx1.  Entries at and past d_nnew[p] keep their bits.  These are the d_pts, d_obs and
 * d_ref of orbm_refresh_map_points_device with d_obs_ptr[k] = 2 * k (one pair: np = d_nnew[p], the arrays offset by
 * p * match_stride, max_obs = 2); one refresh call finishes the new MapPoints.
 *
 * d_mark (NULL = not wanted): [nkf * cap] bytes; every created point stores 1 at d_mark[kf1 * cap + idx1] and
 * d_mark[kf2 * cap + idx2], nothing else is written.  Hand in the array the views' has_mp point into and the next
 * neighbour's orbm_bow_search_device on the same stream sees the reference's state.  As in the reference's loop, the
 * pairs of one current KeyFrame belong in successive calls.  Asynchronous on `stream`. */
typedef enum {
    ORBM_TRI_NO_MATCH = 0,         /* d_match < 0, or idx1 at or past the KeyFrame's count */
    ORBM_TRI_CREATED_SVD = 1,      /* linear triangulation (:321-338) */
    ORBM_TRI_CREATED_STEREO1 = 2,  /* mpCurrentKeyFrame->UnprojectStereo(idx1) (:342) */
    ORBM_TRI_CREATED_STEREO2 = 3,  /* pKF2->UnprojectStereo(idx2) (:346) */
    ORBM_TRI_LOW_PARALLAX = 4,     /* no stereo and very low parallax (:349) */
    ORBM_TRI_W_ZERO = 5,           /* x3D.at<float>(3)==0 (:333) */
    ORBM_TRI_Z1 = 6,               /* z1<=0 (:355) */
    ORBM_TRI_Z2 = 7,               /* z2<=0 (:359) */
    ORBM_TRI_REPROJ1 = 8,          /* reprojection error in the first KeyFrame (:374, :385) */
    ORBM_TRI_REPROJ2 = 9,          /* reprojection error in the second KeyFrame (:400, :411) */
    ORBM_TRI_ZERO_DIST = 10,       /* dist1==0 || dist2==0 (:422) */
    ORBM_TRI_SCALE = 11,           /* scale consistency (:430) */
    ORBM_TRI_INVALID = 12          /* the reference would read out of bounds */
} orbm_triang_status;

orbx_status orbm_triangulate_device(const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_raw, const float* d_uright,
                                    const float* d_depth, const int* d_counts, int nkf, int cap, const float* d_pose,
                                    const int* d_kf_rank, const int* d_pair_a, const int* d_pair_b, int npairs,
                                    const int* d_match, int match_stride, const orbm_pose_params* params, float* d_x3d,
                                    int* d_status, orbm_map_point* d_new_pts, orbm_observation* d_new_obs,
                                    orbm_observation* d_new_ref, int* d_new_idx1, int* d_nnew, uint8_t* d_mark,
                                    void* stream);

/* One pair, host arrays, on HIP device `device`; synchronous.  KeyFrame 1: kps1 (mvKeysUn), kps1_raw (mvKeys; NULL
 * with kps2_raw NULL = the same), uright1 / depth1 (all four stereo arrays NULL = monocular), n1, T1w (12 floats,
 * row-major 3x4 Tcw); likewise KeyFrame 2.  match: n1 ints.  KeyFrame 1 counts as slot 0 and KeyFrame 2 as slot 1 in
 * the observations, and the slot order decides which comes first.  x3d (3 * n1 floats, updated in place), status
 * (n1) and the compacted arrays (room for n1 points; new_obs 2 * n1) as above; only the first *nnew compacted
 * entries are written.  mark1 (n1 bytes) and mark2 (n2 bytes), both or neither, are updated in place. */
orbx_status orbm_triangulate(int device, const orbx_keypoint* kps1, const orbx_keypoint* kps1_raw, const float* uright1,
                             const float* depth1, int n1, const float* T1w, const orbx_keypoint* kps2,
                             const orbx_keypoint* kps2_raw, const float* uright2, const float* depth2, int n2,
                             const float* T2w, const int* match, const orbm_pose_params* params, float* x3d,
                             int* status, orbm_map_point* new_pts, orbm_observation* new_obs,
                             orbm_observation* new_ref, int* new_idx1, int* nnew, uint8_t* mark1, uint8_t* mark2);

/* ---- Local map: Tracking::UpdateLocalMap and the first loop of SearchLocalPoints ----
 * src/Tracking.cc:1283-1391 (UpdateLocalKeyFrames), :1257-1280 (UpdateLocalPoints) and :1198-1214 with the test at
 * :1222, the step of Tracking::TrackLocalMap (:982-992) in front of orbm_frustum_batch_device and
 * orbm_search_by_projection_device.  From a tracked frame's MapPoints it builds mvpLocalKeyFrames, mpReferenceKF and
 * mvpLocalMapPoints and gathers the latter as the d_pts / d_npts / pcap of orbm_frustum_batch_device and the d_pdesc /
 * d_claimed of orbm_search_by_projection_device: the three calls chain on one stream with no host copy.  All integers.
 *
 * KeyFrame table, nkf slots at stride cap (the layout of the calls above): d_counts[nkf]; d_kf_mp[f * cap + i] =
 * GetMapPointMatches()[i] as a MapPoint index or -1; d_kf_bad[f] = isBad(); d_kf_rank[f] = the KeyFrame's position in
 * the caller's std::map<KeyFrame*, ...> order, a permutation of 0..nkf-1 (NULL = slot order, as in
 * orbm_triangulate_device); d_covis[f * 10 ..] = GetBestCovisibilityKeyFrames(10) padded with -1 (as in
 * orbv_db_detect_loop); d_child[d_child_ptr[f] .. d_child_ptr[f + 1]) = GetChilds() in the caller's std::set order;
 * d_parent[f] = GetParent() or -1.
 * MapPoint table, nmp points: d_pts (flags bit 0 = !isBad(), bit 1 = Observations() > 0), d_pdesc[nmp * 32], and
 * d_obs_ptr / d_obs as in orbm_refresh_map_points_device (only .kf is read).
 * Frames, nframes at stride fcap: d_fcounts[fr]; d_frame_mp[fr * fcap + i] = mCurrentFrame.mvpMapPoints[i] or -1, in
 * and out; d_frame_outlier[fr * fcap + i] (NULL = none) = the MapPoint TrackReferenceKeyFrame / TrackWithMotionModel
 * discarded at feature i of this frame (they set its mnLastFrameSeen, :842, :965), or -1.
 *
 * Per frame, as the reference does it:
 *  1 every frame MapPoint that is not bad adds a vote to each KeyFrame of its observation list, bad KeyFrames
 *    included; a bad one is written back as -1 in d_frame_mp (:1286-1303);
 *  2 with no vote at all the reference returns (:1305): d_local_kf[fr * kfcap ..], d_nlocal_kf[fr] and d_ref_kf[fr]
 *    are in and out, hold the previous list and reference KeyFrame on entry and keep them then; otherwise the list
 *    is overwritten;
 *  3 in rank order every voted KeyFrame that is not bad joins the list; pKFmax is the first in rank order with the
 *    most votes (:1315-1330);
 *  4 the expansion runs over those first-stage entries only and stops at the head of an iteration once the list
 *    holds more than 80: per KeyFrame the first covisible that is not bad and not listed, then the first such child,
 *    then the parent if not listed -- whether or not it is bad -- which ends the whole loop (:1334-1384);
 *  5 d_ref_kf[fr] = pKFmax, left as it was when every voted KeyFrame was bad (:1386);
 *  6 over the local KeyFrames in list order and their features in index order, every MapPoint that is not bad is
 *    listed at its first occurrence (:1257-1280);
 *  7 a listed MapPoint that is in the frame's cleaned d_frame_mp or in d_frame_outlier gets flags bit 0 clear
 *    (mnLastFrameSeen == mnId, :1222), every other one set.
 * Outputs per frame: d_local_mp[fr * pcap + k] the MapPoint indices in list order, d_nlocal[fr] their number (at most
 * pcap), d_out_pts[fr * pcap + k] the table's orbm_map_point with flags = (bit 0 of step 7) | (flags & 2),
 * d_out_pdesc[(fr * pcap + k) * 32] its descriptor, d_claimed[fr * fcap + i] = d_frame_mp[i] >= 0 &&
 * Observations() > 0 after step 1, and d_status[fr]: 0 faithful, else a mask of ORBM_LOCAL_MAP_KF_TRUNCATED (the
 * reference's list is longer than kfcap; its first kfcap entries are kept and steps 6-7 use those),
 * ORBM_LOCAL_MAP_POINTS_TRUNCATED (more than pcap MapPoints; the first pcap are written) and ORBM_LOCAL_MAP_INVALID.
 * Invalid: an index the frame reads lies outside its table -- d_fcounts[fr] outside [0, fcap]; a d_frame_mp or
 * d_frame_outlier entry outside [-1, nmp); an observation list of a voting MapPoint that does not ascend from >= 0 or
 * is longer than ORBM_MAX_OBSERVATIONS, or an observation's kf outside [0, nkf); d_kf_rank no permutation; of a
 * KeyFrame the expansion visits a covisible outside [-1, nkf), a child list that does not ascend from >= 0, a child
 * outside [0, nkf) (all its children are checked) or a parent outside [-1, nkf); with no vote d_nlocal_kf[fr] outside
 * [0, kfcap] or a previous entry outside [0, nkf); of a local KeyFrame a count outside [0, cap] or a d_kf_mp entry
 * outside [-1, nmp).  Each is checked before the read it guards, and of an invalid frame nothing but d_status[fr] is
 * written.  Entries at and past the counts keep their bits.
 *
 * d_work: orbm_local_map_work_bytes(nkf, nmp, nframes, kfcap) bytes of device memory, 4-byte aligned, that the caller
 * zeroes once; every call leaves it zeroed again (the entries it touched are put back, so the cost follows the local
 * map, not the whole map) and the calls allocate nothing.  One scratch serves one call at a time.  Vote counters live
 * in LDS up to nkf = ORBM_LOCAL_MAP_LDS_KEYFRAMES and in the scratch beyond.
 * Limits: cap, fcap <= ORBM_MAX_FEATURES, nkf <= ORBV_DB_MAX_KEYFRAMES, kfcap * cap <= INT_MAX (list positions are
 * compared as ints); ORBX_EINVAL otherwise.  Asynchronous on `stream`. */
enum { ORBM_LOCAL_MAP_KF_TRUNCATED = 1, ORBM_LOCAL_MAP_POINTS_TRUNCATED = 2, ORBM_LOCAL_MAP_INVALID = 4 };
#define ORBM_LOCAL_MAP_LDS_KEYFRAMES 8192

/* Pure host code, no device: the scratch size of one call; 0 for arguments the call itself refuses. */
size_t orbm_local_map_work_bytes(int nkf, int nmp, int nframes, int kfcap);

orbx_status orbm_local_map_device(const int* d_counts, const int* d_kf_mp, const uint8_t* d_kf_bad,
                                  const int* d_kf_rank, const int* d_covis, const int* d_child_ptr,
                                  const int* d_child, const int* d_parent, int nkf, int cap,
                                  const orbm_map_point* d_pts, const uint8_t* d_pdesc, const int* d_obs_ptr,
                                  const orbm_observation* d_obs, int nmp, const int* d_fcounts, int* d_frame_mp,
                                  const int* d_frame_outlier, int nframes, int fcap, int* d_local_kf,
                                  int* d_nlocal_kf, int kfcap, int* d_ref_kf, int* d_local_mp, int* d_nlocal,
                                  orbm_map_point* d_out_pts, uint8_t* d_out_pdesc, int pcap, uint8_t* d_claimed,
                                  int* d_status, void* d_work, size_t work_bytes, void* stream);

/* One frame of n features, host arrays, on HIP device `device`; synchronous.  frame_mp (n) and claimed (n), local_kf
 * (kfcap) with *nlocal_kf and *ref_kf in and out, local_mp / out_pts / out_pdesc with room for pcap points; what the
 * device form leaves untouched keeps its bits here too.  ORBX_EINVAL when child_ptr or obs_ptr does not ascend from
 * >= 0.  The scratch is the call's own. */
orbx_status orbm_local_map(int device, const int* counts, const int* kf_mp, const uint8_t* kf_bad, const int* kf_rank,
                           const int* covis, const int* child_ptr, const int* child, const int* parent, int nkf,
                           int cap, const orbm_map_point* pts, const uint8_t* pdesc, const int* obs_ptr,
                           const orbm_observation* obs, int nmp, int n, int* frame_mp, const int* frame_outlier,
                           int* local_kf, int* nlocal_kf, int kfcap, int* ref_kf, int* local_mp, int* nlocal,
                           orbm_map_point* out_pts, uint8_t* out_pdesc, int pcap, uint8_t* claimed, int* status);

/* ---- The covisibility graph: KeyFrame::UpdateConnections and what hangs on it ----
 * src/KeyFrame.cc:289-379 (UpdateConnections) with AddConnection (:123-136) and UpdateBestCovisibles (:138-157), the
 * connection part of SetBadFlag (:466-467, :476-477) with EraseConnection (:553-567), and the getters
 * GetBestCovisibilityKeyFrames (:174-182), GetConnectedKeyFrames (:159-166), GetCovisiblesByWeight (:184-199) and
 * GetChilds.  The graph lives in caller-owned device memory beside the KeyFrame and MapPoint tables of
 * orbm_local_map_device, is updated in place from the observation lists the refresh and the triangulation keep
 * current, and the getters write the d_covis / d_child_ptr / d_child / d_connected tables orbm_local_map_device and
 * orbv_db_detect_*_device take: the calls chain on one stream with no host copy.  All integers.
 *
 * nkf slots at row stride ccap <= ORBM_MAX_CONNECTIONS; all arrays are read and written in place, and entries at and
 * past the counts keep their bits. */
typedef struct {
    int32_t* conn_kf;   /* [nkf * ccap] mConnectedKeyFrameWeights of slot f at f * ccap: the KeyFrames, every voted one
                           (also below the threshold, :367), in ascending slot order, none twice */
    int32_t* conn_w;    /* [nkf * ccap] their weights */
    int32_t* nconn;     /* [nkf] the map's size */
    int32_t* ord_kf;    /* [nkf * ccap] mvpOrderedConnectedKeyFrames: descending weight, among equal weights descending
                           d_kf_rank (the reference sorts ascending on (weight, pointer) and pushes to the front,
                           :146-156, :354-361) */
    int32_t* ord_w;     /* [nkf * ccap] mvOrderedWeights */
    int32_t* nord;      /* [nkf] their length */
    int32_t* parent;    /* [nkf] mpParent or -1 */
    uint8_t* first;     /* [nkf] mbFirstConnection */
} orbm_covis_graph;

#define ORBM_MAX_CONNECTIONS 4096

/* KeyFrame::UpdateConnections for d_targets[0 .. ntargets) as if called one after another in that order (a slot may
 * repeat; the targets run as launches in sequence on `stream`, and no result is read on the host).  `graph` is a host
 * struct of device pointers.  The KeyFrame table (d_counts, d_kf_mp at stride cap, d_kf_rank or NULL = slot order) and
 * the MapPoint table (d_pts, d_obs_ptr, d_obs, nmp) are those of orbm_local_map_device; of an orbm_map_point only
 * flags bit 0 is read, of an observation only .kf.  th >= 1 is the reference's 15 (:330); root is the slot whose
 * mnId is 0, or -1.
 *
 * Per target t, as the reference does it:
 *  1 every MapPoint of t that is not NULL and not bad adds a vote to each KeyFrame of its observation list but t
 *    itself (slot equality stands for mnId==mnId, :316); a bad KeyFrame is counted, isBad() is not asked (:302-320);
 *  2 with no vote at all the reference returns (:323): nothing of the graph is written, d_status = ORBM_CONN_EMPTY;
 *  3 over the voted KeyFrames in ascending rank pKFmax is the first with the strictly largest count; every KeyFrame
 *    with count >= th enters vPairs and receives AddConnection(t, count); if none does, pKFmax alone (:328-352);
 *  4 AddConnection(n <- t, w) (:123-136) inserts t into n's map, or overwrites a different weight; with an equal
 *    weight nothing changes and n's ordered list is NOT rebuilt; after an insert or overwrite UpdateBestCovisibles
 *    (:138-157) rebuilds n's ordered list from its WHOLE map, entries below th included;
 *  5 t's map becomes all voted KeyFrames with their counts, its ordered list vPairs only (:354-369); a KeyFrame t was
 *    connected to before and no longer votes for keeps its stale entry for t -- the reference erases nothing here;
 *  6 if first[t] is set and t != root: parent[t] = ord_kf[t][0], first[t] = 0 (:371-376); otherwise both stand.
 *
 * d_status[i], per position in d_targets: 0 faithful; ORBM_CONN_EMPTY (step 2); ORBM_CONN_NOSPC: t's map, or the map
 * of a neighbour that needs an insert, would exceed ccap; ORBM_CONN_INVALID: the reference would read out of bounds --
 * the target outside [0, nkf); d_counts[t] outside [0, cap]; a d_kf_mp entry outside [-1, nmp); an observation list of
 * a voting MapPoint that does not ascend from >= 0 or is longer than ORBM_MAX_OBSERVATIONS; an observation's kf
 * outside [0, nkf); d_kf_rank no permutation; of a row the call reads -- the map row of every vPairs neighbour -- nconn
 * outside [0, ccap] or an entry outside [0, nkf).  When t's own map exceeds ccap the neighbours' rows are not read;
 * otherwise an invalid neighbour row outranks a full one.  Each read is checked before it is made, and the status is
 * decided before the first write: for NOSPC and INVALID nothing but d_status[i] is written, neighbour rows included.
 * Later targets still run.  What keeps its bits: every row and count of a KeyFrame that is neither t nor a neighbour
 * that received an insert or overwrite, row entries at and past the new counts, parent / first unless step 6 applies.
 *
 * d_work: orbm_connections_work_bytes(nkf, ccap) bytes of device memory, 4-byte aligned, that the caller zeroes once;
 * every call leaves it zeroed again and the calls allocate nothing.  One scratch serves one call at a time.  Vote
 * counters live in LDS up to nkf = ORBM_LOCAL_MAP_LDS_KEYFRAMES and in the scratch beyond.
 * Limits: nkf <= ORBV_DB_MAX_KEYFRAMES, cap <= ORBM_MAX_FEATURES, 1 <= ccap <= ORBM_MAX_CONNECTIONS, th >= 1, root in
 * [-1, nkf); ORBX_EINVAL otherwise.  Asynchronous on `stream`. */
enum { ORBM_CONN_EMPTY = 1, ORBM_CONN_NOSPC = 2, ORBM_CONN_INVALID = 4 };

/* Pure host code, no device: the scratch size of one call; 0 for arguments the call itself refuses. */
size_t orbm_connections_work_bytes(int nkf, int ccap);

orbx_status orbm_update_connections_device(const orbm_covis_graph* graph, int nkf, int ccap, const int* d_counts,
                                           const int* d_kf_mp, int cap, const int* d_kf_rank,
                                           const orbm_map_point* d_pts, const int* d_obs_ptr,
                                           const orbm_observation* d_obs, int nmp, const int* d_targets, int ntargets,
                                           int th, int root, int* d_status, void* d_work, size_t work_bytes,
                                           void* stream);

/* The same on host arrays (`graph` holds host pointers, read and written in place), on HIP device `device`;
 * synchronous.  The argument checks run before any device call.  ORBX_EINVAL also when obs_ptr does not ascend from
 * >= 0 or nkf < 1.  What the device form leaves untouched keeps its bits here too.  The scratch is the call's own. */
orbx_status orbm_update_connections(int device, const orbm_covis_graph* graph, int nkf, int ccap, const int* counts,
                                    const int* kf_mp, int cap, const int* kf_rank, const orbm_map_point* pts,
                                    const int* obs_ptr, const orbm_observation* obs, int nmp, const int* targets,
                                    int ntargets, int th, int root, int* status);

/* The connection part of KeyFrame::SetBadFlag (:466-467, :476-477) for d_targets in sequence: for every n in t's map,
 * EraseConnection (:553-567) -- if n's map holds t, t is removed (the row closes up) and n's ordered list is rebuilt
 * from its whole map; otherwise n is left alone -- then nconn[t] = nord[t] = 0; t's row entries keep their bits.  An
 * entry of t's map that names t itself is skipped.  d_status[i]: 0, or ORBM_CONN_INVALID when the target is outside
 * [0, nkf), d_kf_rank is no permutation, nconn[t] is outside [0, ccap], an entry of t's row is outside [0, nkf), or
 * the row of one of them has such a count or entry; checked before the reads they guard, and then nothing but
 * d_status[i] is written.  The mbNotErase test, the observation erasure, the spanning-tree repair (:480-537) and the
 * database erase stay with the caller.  d_work as above.  Asynchronous on `stream`. */
orbx_status orbm_erase_connections_device(const orbm_covis_graph* graph, int nkf, int ccap, const int* d_kf_rank,
                                          const int* d_targets, int ntargets, int* d_status, void* d_work,
                                          size_t work_bytes, void* stream);

/* The getters, asynchronous on `stream`; a nord / nconn outside [0, ccap] is clamped into it before the row is read.
 * d_out[f * N + j] = GetBestCovisibilityKeyFrames(N)[j] of every slot, padded with -1 (:174-182): with N = 10 the
 * d_covis of orbm_local_map_device and orbv_db_detect_*_device.  1 <= N <= ORBM_MAX_CONNECTIONS. */
orbx_status orbm_best_covisibles_device(const orbm_covis_graph* graph, int nkf, int ccap, int N, int* d_out,
                                        void* stream);

/* d_mask[nkf] = 1 where the slot is in GetConnectedKeyFrames() of t (:159-166), else 0: the d_connected of
 * orbv_db_detect_loop_device.  A map entry outside [0, nkf) marks nothing.  t in [0, nkf). */
orbx_status orbm_connected_mask_device(const orbm_covis_graph* graph, int nkf, int ccap, int t, uint8_t* d_mask,
                                       void* stream);

/* d_n[f] = the length GetCovisiblesByWeight(w) returns (:184-199): the index of the first ordered weight < w, and 0
 * when there is none -- upper_bound hits end() when every weight is >= w, and the reference returns an empty vector
 * then (:192).  The list is d_ord_kf[f * ccap .. + d_n[f]). */
orbx_status orbm_covisibles_by_weight_device(const orbm_covis_graph* graph, int nkf, int ccap, int w, int* d_n,
                                             void* stream);

/* GetChilds() of every slot as the CSR orbm_local_map_device reads: d_child[d_child_ptr[f] .. d_child_ptr[f + 1]) =
 * {c : d_parent[c] == f and not d_kf_bad[c]} in ascending d_kf_rank (NULL = slot order), the std::set<KeyFrame*>
 * order; d_child_ptr has nkf + 1 entries, d_child room for nkf.  This equals mspChildrens for every KeyFrame that is
 * not bad: AddChild is called where the parent is set (:374, :397) and EraseChild only by a KeyFrame turning bad
 * (:537); a bad KeyFrame's own set may be stale in the reference, and the local-map expansion asks it only of
 * KeyFrames that are not bad.  *d_status (one int): 0, or ORBM_CONN_INVALID when a parent is outside [-1, nkf) or
 * d_kf_rank is no permutation; then nothing else is written.  d_work: orbm_children_work_bytes(nkf) bytes, zeroed
 * once by the caller and left zeroed by every call.  A child's place is found by counting its siblings of lower
 * rank: the cost grows with the square of a KeyFrame's children.  Asynchronous on `stream`. */
size_t orbm_children_work_bytes(int nkf);

orbx_status orbm_children_device(const int* d_parent, const uint8_t* d_kf_bad, const int* d_kf_rank, int nkf,
                                 int* d_child_ptr, int* d_child, int* d_status, void* d_work, size_t work_bytes,
                                 void* stream);

/* ---- LocalMapping's culls: MapPointCulling and KeyFrameCulling ----
 * src/LocalMapping.cc:170-205 and :632-696 with the observation-side edits they cause: MapPoint::SetBadFlag
 * (src/MapPoint.cc:151-168), MapPoint::EraseObservation (:111-137), MapPoint::GetFoundRatio (:236-240),
 * KeyFrame::EraseMapPointMatch (src/KeyFrame.cc:222-227) and the tests and the observation loop of
 * KeyFrame::SetBadFlag (:457-464, :469-471).  They run over the KeyFrame and MapPoint tables of
 * orbm_local_map_device / orbm_update_connections_device, in place, so that the culls, the compaction, the erase of
 * the culled KeyFrames' connections, the refresh and the next local map chain on one stream with no host copy.
 *
 * Tables: d_counts, d_kf_mp at stride cap (in and out), d_pts (flags in and out), d_obs_ptr / d_obs, d_ref as in
 * orbm_refresh_map_points_device (in and out).  List order is the caller's std::map order; a list's live entries name
 * distinct KeyFrames, as a std::map's keys do (not checked).  New columns: d_nobs[nmp] = the nObs counter of
 * Observations(), a stereo observation counted twice (in and out); d_uright / d_depth = mvuRight / mvDepth at stride
 * cap (d_uright NULL = monocular, all -1); d_kps = mvKeysUn at stride cap (only .octave is read); d_found, d_visible,
 * d_first_kfid [nmp] = mnFound, mnVisible, mnFirstKFid; d_kf_noterase[nkf] = mbNotErase.
 *
 * Erased mask: d_obs_erased[d_obs_ptr[nmp]] bytes, in and out.  An entry whose byte is not 0 does not exist for any of
 * these calls: whatever it holds has no effect and is not range-checked.  The calls never move an entry of d_obs, they
 * set bytes, so the list order that decides the refresh's ties stands and the two culls run back to back;
 * orbm_compact_observations_device then writes the CSR the other calls read.  Also not checked: a list's live entries
 * name distinct KeyFrames, as a std::map's keys do; only a list that names a culled candidate twice makes an outcome
 * depend on the order of execution.
 *
 * Range checks, each before the read it guards.  A list that does not ascend from >= 0 or is longer than
 * ORBM_MAX_OBSERVATIONS, and a live observation whose kf is outside [0, nkf) or whose idx is outside
 * [0, min(d_counts[kf], cap)), make the unit that walks the list -- a recent MapPoint, a candidate KeyFrame -- INVALID:
 * its verdict is written and nothing else of it, and later units still run.  Every live entry of a walked list is
 * checked, also where the reference leaves its loop early.  Limits: nkf <= ORBV_DB_MAX_KEYFRAMES, cap <=
 * ORBM_MAX_FEATURES, 1 <= ccap <= ORBM_MAX_CONNECTIONS, nlevels in [1, 16], t in [0, nkf), root in [-1, nkf);
 * ORBX_EINVAL otherwise, and for a NULL table.  All asynchronous on `stream`; nothing is allocated or read on the host.
 *
 * MapPointCulling over mlpRecentAddedMapPoints = d_recent[0 .. nrecent), MapPoint indices, each listed once;
 * cur_kfid = mpCurrentKeyFrame->mnId, th_obs = 2 (monocular) or 3.  d_verdict[k], tested in the reference's order:
 * ERASED_BAD flags bit 0 clear (:186); RATIO (float)found / (float)visible < 0.25f, the division correctly rounded, a
 * NaN or +inf comparing false (:190); OBS (int)cur_kfid - (int)first_kfid >= 2 && nobs <= th_obs (:195); DROPPED_OLD
 * that difference >= 3 (:200); KEPT; INVALID the index outside [0, nmp), or, for RATIO and OBS, a list check.  RATIO and
 * OBS run SetBadFlag: flags bit 0 clears, every live observation (kf, idx) stores -1 at d_kf_mp[kf * cap + idx]
 * whatever stands there (EraseMapPointMatch) and has its mask byte set; d_nobs keeps its value, as in the reference,
 * and with it flags bit 1.  d_recent_out[0 .. *d_nrecent_out) = the KEPT points in list order (room for nrecent). */
enum {
    ORBM_CULL_KEPT = 0,
    ORBM_CULL_ERASED_BAD = 1,
    ORBM_CULL_RATIO = 2,
    ORBM_CULL_OBS = 3,
    ORBM_CULL_DROPPED_OLD = 4,
    ORBM_CULL_INVALID = 5
};

orbx_status orbm_map_point_culling_device(const int* d_recent, int nrecent, int cur_kfid, int th_obs,
                                          const int* d_counts, int* d_kf_mp, int nkf, int cap, orbm_map_point* d_pts,
                                          const int* d_obs_ptr, const orbm_observation* d_obs, uint8_t* d_obs_erased,
                                          int nmp, const int* d_nobs, const int* d_found, const int* d_visible,
                                          const int* d_first_kfid, int* d_verdict, int* d_recent_out,
                                          int* d_nrecent_out, void* stream);

/* KeyFrameCulling of KeyFrame t.  The candidates are ord_kf[t][0 .. nord[t]) of `graph` (a host struct of device
 * pointers; only ord_kf and nord are read) as they are when the call runs, GetVectorCovisibleKeyFrames(), and they are
 * processed as if one after another: a candidate sees every edit of the ones before it.  Per candidate c:
 *  1 c == root: SKIP_ROOT (:643); nothing is counted;
 *  2 for every feature i < d_counts[c] with mp = d_kf_mp[c * cap + i] >= 0 and flags bit 0 set: with `stereo`
 *    (!mbMonocular) a feature with depth > th_depth || depth < 0 is skipped (float compares: a NaN depth is counted);
 *    otherwise nMPs++, and if d_nobs[mp] > 3 the live observations with kf != c and octave(kf, idx) <=
 *    octave(c, i) + 1 are counted: three or more make the feature redundant (:651-691);
 *  3 the KeyFrame is culled iff (double)nRed > 0.9 * (double)nMPs (:693);
 *  4 a culled c with d_kf_noterase[c] set: TO_BE_ERASED and no edit (mbToBeErased, KeyFrame.cc:459-463);
 *  5 CULLED otherwise: for every feature with mp >= 0, isBad() not asked (:470), the first live entry of mp's list
 *    with kf == c, if any, is erased -- once per MapPoint, however many features of c name it: d_nobs[mp] -=
 *    (d_uright[c * cap + that entry's idx] >= 0 ? 2 : 1); if d_ref[mp].kf == c, d_ref[mp] = the first remaining live
 *    entry (left as it was when none remains); flags bit 1 = d_nobs[mp] > 0; if d_nobs[mp] <= 2, SetBadFlag as above
 *    over the remaining entries.  d_kf_mp[c * cap + i] itself keeps naming the point.
 * INVALID: c outside [0, nkf); d_counts[c] outside [0, cap]; a d_kf_mp[c] entry outside [-1, nmp); a list check of a
 * list step 2 or step 5 walks; in step 2 an octave outside [0, nlevels), of feature i or of a counted observation.
 * The checks of step 5 run before its first write.  nord[t] outside [0, ccap]: *d_ncand = -1, nothing is processed.
 * Outputs: d_verdict[j] per candidate; d_nmps[j] and d_nred[j] for KEPT, CULLED and TO_BE_ERASED; d_culled[j] = c for
 * CULLED and -1 otherwise, all ccap entries, which is the target list of orbm_erase_connections_device (a -1 target is
 * ORBM_CONN_INVALID there and writes nothing); *d_nculled; *d_ncand = nord[t].  d_kf_bad, the connections, the
 * spanning tree, mTcp and the Map / database erase stay with the caller; the verdict loop reads none of them.
 * d_work: orbm_culling_work_bytes(nmp) bytes, 4-byte aligned, zeroed once by the caller and left zeroed by every
 * call.  One workgroup walks the candidates: the cost grows with their number times a KeyFrame's features. */
enum {
    ORBM_KFCULL_KEPT = 0,
    ORBM_KFCULL_SKIP_ROOT = 1,
    ORBM_KFCULL_CULLED = 2,
    ORBM_KFCULL_TO_BE_ERASED = 3,
    ORBM_KFCULL_INVALID = 4
};

/* Pure host code, no device: the scratch size of one call; 0 for arguments the call itself refuses. */
size_t orbm_culling_work_bytes(int nmp);

orbx_status orbm_keyframe_culling_device(const orbm_covis_graph* graph, int nkf, int ccap, int t, int root,
                                         const int* d_counts, int* d_kf_mp, int cap, const orbx_keypoint* d_kps,
                                         const float* d_uright, const float* d_depth, float th_depth, int stereo,
                                         int nlevels, const uint8_t* d_kf_noterase, orbm_map_point* d_pts,
                                         const int* d_obs_ptr, const orbm_observation* d_obs, uint8_t* d_obs_erased,
                                         orbm_observation* d_ref, int* d_nobs, int nmp, int* d_verdict, int* d_nmps,
                                         int* d_nred, int* d_culled, int* d_nculled, int* d_ncand, void* d_work,
                                         size_t work_bytes, void* stream);

/* The stable compaction of (d_obs_ptr, d_obs, d_obs_erased): d_obs_ptr_out[nmp + 1] and d_obs_out (room for
 * d_obs_ptr[nmp] entries) hold every live entry in list order -- the CSR the refresh, the local map and
 * UpdateConnections read next.  Entries of d_obs_out past the new total keep their bits.  *d_status: 0, or
 * ORBM_CONN_INVALID when a list does not ascend from >= 0 or is longer than ORBM_MAX_OBSERVATIONS; such a list is
 * compacted as an empty one. */
orbx_status orbm_compact_observations_device(const int* d_obs_ptr, const orbm_observation* d_obs,
                                             const uint8_t* d_obs_erased, int nmp, int* d_obs_ptr_out,
                                             orbm_observation* d_obs_out, int* d_status, void* stream);

/* The same on host arrays, updated in place, on HIP device `device`; synchronous.  The argument checks run before any
 * device call.  ORBX_EINVAL also when obs_ptr does not ascend from >= 0 or nkf < 1 (and, for the compaction, when a
 * list is longer than ORBM_MAX_OBSERVATIONS).  What the device form leaves untouched keeps its bits here too.  `graph`
 * holds host pointers, of which ord_kf and nord are read; verdict, nmps, nred and culled have ccap entries.  The
 * scratch is the call's own. */
orbx_status orbm_map_point_culling(int device, const int* recent, int nrecent, int cur_kfid, int th_obs,
                                   const int* counts, int* kf_mp, int nkf, int cap, orbm_map_point* pts,
                                   const int* obs_ptr, const orbm_observation* obs, uint8_t* obs_erased, int nmp,
                                   const int* nobs, const int* found, const int* visible, const int* first_kfid,
                                   int* verdict, int* recent_out, int* nrecent_out);

orbx_status orbm_keyframe_culling(int device, const orbm_covis_graph* graph, int nkf, int ccap, int t, int root,
                                  const int* counts, int* kf_mp, int cap, const orbx_keypoint* kps,
                                  const float* uright, const float* depth, float th_depth, int stereo, int nlevels,
                                  const uint8_t* kf_noterase, orbm_map_point* pts, const int* obs_ptr,
                                  const orbm_observation* obs, uint8_t* obs_erased, orbm_observation* ref, int* nobs,
                                  int nmp, int* verdict, int* nmps, int* nred, int* culled, int* nculled, int* ncand);

orbx_status orbm_compact_observations(int device, const int* obs_ptr, const orbm_observation* obs,
                                      const uint8_t* obs_erased, int nmp, int* obs_ptr_out,
                                      orbm_observation* obs_out, int* status);

/* ---- DBoW2 vocabulary (TemplatedVocabulary, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) ----
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:521-528, src/KeyFrame.cc:59-66) call
 * transform(descriptors, mBowVec, mFeatVec, 4); the FeatureVector it produces is the
 * candidate set of the SearchByBoW / SearchForTriangulation entry points above. */
typedef struct orbx_vocabulary orbx_vocabulary;

/* TemplatedVocabulary::loadFromTextFile (:1338-1424): header "k L scoring weighting", then one
 * node per line "parent is_leaf d0 .. d31 weight" (node ids 1, 2, ... in file order). */
orbx_status orbv_load_text(const char* path, int device, orbx_vocabulary** out);

/* The same vocabulary from arrays: nnodes entries including the root (index 0, whose
 * parent / is_leaf / descriptor / weight are ignored); parent[i] < i. */
orbx_status orbv_create(int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                        orbx_vocabulary** out);
void orbv_destroy(orbx_vocabulary* v);
orbx_status orbv_info(const orbx_vocabulary* v, int* k, int* L, int* scoring, int* weighting, int* nnodes,
                      int* nwords);

/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (:1125-1259) for
 * one host descriptor set (n <= ORBV_MAX_FEATURES).  BowVector: bow_n words ascending with their weights
 * (n entries of room); FeatureVector as CSR: fv_nnodes node ids ascending, fv_ptr (n + 1),
 * fv_idx (n).  Synchronous. */
orbx_status orbv_transform(const orbx_vocabulary* v, const uint8_t* desc, int n, int levelsup, int32_t* bow_word,
                           double* bow_weight, int* bow_n, int32_t* fv_node, int32_t* fv_ptr, int32_t* fv_idx,
                           int* fv_nnodes);

/* Batched device path over an extract batch (d_desc [nframes][cap][32], d_counts[nframes],
 * cap <= ORBV_MAX_FEATURES).  Per frame f: d_bow_word / d_bow_weight / d_fv_node / d_fv_idx at f * cap,
 * d_fv_ptr at f * (cap + 1), counts d_bow_n[f] / d_fv_nnodes[f].  The FeatureVector CSR
 * plugs straight into orbm_bow_view.  Asynchronous on `stream`. */
orbx_status orbv_transform_batch_device(const orbx_vocabulary* v, const uint8_t* d_desc, const int* d_counts,
                                        int nframes, int cap, int levelsup, int32_t* d_bow_word,
                                        double* d_bow_weight, int* d_bow_n, int32_t* d_fv_node, int32_t* d_fv_ptr,
                                        int32_t* d_fv_idx, int* d_fv_nnodes, void* stream);

/* ---- KeyFrameDatabase (src/KeyFrameDatabase.cc) and TemplatedVocabulary::score ----
 * The step between orbv_transform* and the candidate-driven searches above: which keyframes to hand to
 * SearchByBoW.  BowVectors are what orbv_transform writes: int32_t word ids ascending, double weights.
 * Only L1_NORM (scoring 0) is served, the scoring ORBvoc carries and ORB_SLAM2 never changes: the other DBoW2
 * scorings sum vi * wi products, whose FMA contraction in the reference's -O3 -march=native build is not pinned,
 * and KL needs log.  orbv_score with another scoring and orbv_db_create on another vocabulary return ORBX_EINVAL.
 *
 * Limits: qn and every keyframe's n <= ORBV_MAX_FEATURES; at most ORBV_DB_MAX_KEYFRAMES slots between clears,
 * erased ones included (ORBX_ENOSPC from add beyond).  Word ids must lie in [0, nwords) and ascend strictly; the
 * host entry points check this (ORBX_EINVAL), the _device forms take the transform's output as it is.
 * Threading: calls on one database serialise on an internal mutex, as the reference's mMutex does (Tracking,
 * LocalMapping and LoopClosing all call it).  The database owns a non-blocking stream for its storage; the
 * synchronous calls run on the pooled streams of the other host calls; every call leaves the caller's current
 * device as found. */
#define ORBV_DB_MAX_KEYFRAMES 65536

/* TemplatedVocabulary::score -> L1Scoring::score (ScoringObject.cpp:23-68).  Pure host code, no device. */
orbx_status orbv_score(int scoring, const int32_t* word1, const double* weight1, int n1, const int32_t* word2,
                       const double* weight2, int n2, double* score);

typedef struct orbv_database orbv_database;
/* KeyFrameDatabase(voc), on the vocabulary's device.  reserve_* = initial room (0 = defaults); storage grows on
 * demand (doubling, device-to-device copies). */
orbx_status orbv_db_create(const orbx_vocabulary* v, int reserve_keyframes, int reserve_words, orbv_database** out);
void orbv_db_destroy(orbv_database* db);
/* KeyFrameDatabase::add (:40-46): returns the keyframe's slot = its position in add order (0, 1, ...).  The
 * slot's mLoopScore / mRelocScore start at 0.0f.  Synchronous. */
orbx_status orbv_db_add(orbv_database* db, const int32_t* bow_word, const double* bow_weight, int n, int* slot);
/* The same for frames 0..nframes-1 of an orbv_transform_batch_device result (f * cap layout), slots[nframes] out
 * (host, may be NULL).  Waits on `stream` for the nframes counts and for the copy (keyframe insertion is not a
 * per-frame path). */
orbx_status orbv_db_add_batch_device(orbv_database* db, const int32_t* d_bow_word, const double* d_bow_weight,
                                     const int* d_bow_n, int nframes, int cap, int* slots, void* stream);
/* KeyFrameDatabase::erase (:48-67): the slot keeps its number and its storage until clear; it never shares a
 * word again and so is skipped as a neighbour. */
orbx_status orbv_db_erase(orbv_database* db, int slot);
/* KeyFrameDatabase::clear (:69-73): slots restart at 0. */
orbx_status orbv_db_clear(orbv_database* db);
/* nslots: slots handed out since the last clear; nlive: those not erased; words_stored: BowVector entries held. */
orbx_status orbv_db_info(const orbv_database* db, int* nslots, int* nlive, size_t* words_stored);
/* LoopClosing::DetectLoop's reference-score loop (src/LoopClosing.cc:124-138): score(query, slot) as double for
 * each listed slot (an erased slot scores 0); the caller skips isBad() and takes the min as float. */
orbx_status orbv_db_scores(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn, const int* slots,
                           int ns, double* scores);
/* DetectLoopCandidates(pKF, minScore) (:76-197) / DetectRelocalizationCandidates(F) (:199-309).  With nslots the
 * database's slot count:
 *   connected[nslots]   spConnectedKeyFrames.count(slot); NULL = none.
 *   covis[nslots * 10]  GetBestCovisibilityKeyFrames(10) of each slot as slots, in that order, padded with -1; a
 *                       neighbour that is not in the database is -1; NULL = no neighbours.
 *   cand[cap]           vpLoopCandidates / vpRelocCandidates as slots, in the reference's order; ORBX_ENOSPC with
 *                       *ncand set (and the first cap candidates written) when cap is too small.
 *   words[nslots]       (optional) mnLoopWords / mnRelocWords of the slots in lKFsSharingWords, 0 for every other
 *                       slot (the reference leaves 1 in a connected keyframe and never reads it).
 *   scores[nslots]      (optional) mLoopScore / mRelocScore of every slot as the reference's keyframes hold them
 *                       after the call.  They are per-slot state of the database and persist across queries:
 *                       DetectRelocalizationCandidates adds pKF2->mRelocScore of any neighbour that merely shares
 *                       a word (:273-276), scored in this query or not, so it reads what an earlier query left.
 *                       That stale read is reproduced; where the reference's member is indeterminate (never
 *                       scored) it is 0.0f here (set by add).  The loop form asks mnLoopWords > minCommonWords of
 *                       a neighbour and so only reads fresh scores.
 * Synchronous. */
orbx_status orbv_db_detect_loop(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn,
                                const uint8_t* connected, const int32_t* covis, float min_score, int* cand, int cap,
                                int* ncand, int* words, float* scores);
orbx_status orbv_db_detect_reloc(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn,
                                 const int32_t* covis, int* cand, int cap, int* ncand, int* words, float* scores);
/* _device forms: every pointer a device pointer, the query being one frame of a transform batch (its d_bow_word /
 * d_bow_weight rows of q_cap entries and its count d_qn -> one int, clamped to q_cap <= ORBV_MAX_FEATURES).
 * nslots = the database's slot count (ORBX_EINVAL otherwise); d_cand has nslots entries, d_ncand one; d_words /
 * d_scores (nslots each) may be NULL.  Asynchronous on `stream`; no host read of any result.  Later calls on the
 * database, on any stream, are ordered behind it. */
orbx_status orbv_db_detect_loop_device(orbv_database* db, const int32_t* d_q_word, const double* d_q_weight,
                                       const int* d_qn, int q_cap, const uint8_t* d_connected,
                                       const int32_t* d_covis, float min_score, int nslots, int* d_cand,
                                       int* d_ncand, int* d_words, float* d_scores, void* stream);
orbx_status orbv_db_detect_reloc_device(orbv_database* db, const int32_t* d_q_word, const double* d_q_weight,
                                        const int* d_qn, int q_cap, const int32_t* d_covis, int nslots, int* d_cand,
                                        int* d_ncand, int* d_words, float* d_scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif
