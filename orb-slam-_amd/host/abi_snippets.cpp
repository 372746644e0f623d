// Compile check of INTEGRATION.md: every C ABI call the document shows, with the document's argument
// lists and plain types standing in for cv::Mat / cv::KeyPoint / the ORB-SLAM2 objects.  Built (not run)
// by the Makefile, so a snippet that drifts from include/orbx.h breaks the build.
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/orbx.h"

namespace {

struct KeyPoint {   // cv::KeyPoint
    float x, y, size, angle, response;
    int octave, class_id;
};
struct Point2f {
    float x, y;
};
static_assert(sizeof(KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint layout");

int snippets(orbx_handle* h, orbx_handle* hl, orbx_handle* hr, orbx_vocabulary* vocab_handle, void* stream)
{
    // section 2: ORBextractor adapter
    int nfeatures = 2000, nlevels = 8, iniThFAST = 20, minThFAST = 7;
    float scaleFactor = 1.2f;
    orbx_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
    orbx_handle* created = nullptr;
    orbx_create(&p, /*device*/ 0, &created);
    std::vector<float> sf(8), isf(8), s2(8), is2(8);
    std::vector<int> fpl(8);
    orbx_get_tables(h, nullptr, nullptr, sf.data(), isf.data(), s2.data(), is2.data(), fpl.data());
    orbx_set_cv_modes(h, ORBX_RESIZE_SSE2, ORBX_BLUR_SSE2);
    orbx_set_cv_modes(h, ORBX_RESIZE_SSE2, ORBX_BLUR_BITEXACT);
    int rows = 376, cols = 1241, cap = orbx_capacity(h, rows, cols), n = 0;
    std::vector<uint8_t> image((size_t)rows * cols), desc((size_t)cap * 32);
    std::vector<KeyPoint> kps(cap);
    orbx_extract(h, image.data(), rows, cols, (size_t)cols, (orbx_keypoint*)kps.data(), cap, desc.data(), &n);
    const uint8_t* d;
    int r, c;
    size_t s;
    orbx_get_level(h, 0, &d, &r, &c, &s);

    // image ingest
    const uint8_t* d_raw = nullptr;
    const float *d_mx = nullptr, *d_my = nullptr;
    uint8_t* d_gray = nullptr;
    orbx_keypoint* d_kps = nullptr;
    uint8_t* d_desc = nullptr;
    int* d_counts = nullptr;
    int batch = 2, channels = 3, mbRGB = 0, rows_rect = 480, cols_rect = 752;
    orbx_ingest_batch_device(d_raw, batch, rows, cols, channels, mbRGB, cols * channels, (size_t)rows * cols * channels,
                             d_mx, d_my, 2, rows_rect, cols_rect, d_gray, cols_rect, (size_t)rows_rect * cols_rect,
                             stream);
    orbx_extract_batch_device(h, d_gray, batch, rows_rect, cols_rect, cols_rect, (size_t)rows_rect * cols_rect, d_kps,
                              d_desc, d_counts, cap, stream);
    const void* d_depth16 = nullptr;
    float* d_depth = nullptr;
    float mDepthMapFactor = 1.f / 5000;
    orbx_depth_batch_device(d_depth16, 0, batch, rows, cols, 2 * cols, 2 * rows * cols, mDepthMapFactor, d_depth,
                            4 * cols, 4 * rows * cols, stream);

    // the Frame constructors
    float fx = 435.2f, fy = 435.2f, cx = 367.2f, cy = 252.2f, k1 = -0.28f, k2 = 0.07f, tp1 = 0.f, tp2 = 0.f, k3 = 0.f;
    float mbf = 47.9f;
    const orbx_camera cam{fx, fy, cx, cy, k1, k2, tp1, tp2, k3};   // mDistCoef = k1 k2 p1 p2 k3
    float bounds[4];
    orbx_image_bounds(&cam, rows, cols, bounds);
    const orbm_grid gb{bounds[0], bounds[2], 64.f / (bounds[1] - bounds[0]), 48.f / (bounds[3] - bounds[2])};
    std::vector<float> xy(2 * (size_t)n);
    int N = n;
    orbx_undistort_points(&cam, xy.data(), N, xy.data());
    orbx_keypoint* d_kps_un = nullptr;
    const int *d_left = nullptr, *d_right = nullptr;
    float *d_uright = nullptr, *d_depth_kp = nullptr;
    int* d_ngood = nullptr;
    orbx_undistort_batch_device(d_kps, d_counts, batch, cap, &cam, d_kps_un, stream);
    orbx_stereo_batch_device(h, d_kps, d_desc, d_counts, cap, d_left, d_right, batch / 2, mbf, fx, d_uright, d_depth_kp,
                             d_ngood, stream);
    orbx_rgbd_stereo_batch_device(d_kps, d_kps_un, d_counts, batch, cap, d_depth, rows, cols, 4 * cols,
                                  (size_t)4 * rows * cols, mbf, d_uright, d_depth_kp, stream);
    std::vector<float> imDepth((size_t)rows * cols), uR(n), dK(n);
    orbx_rgbd_stereo(0, (const orbx_keypoint*)kps.data(), (const orbx_keypoint*)kps.data(), N, imDepth.data(), rows,
                     cols, 4 * (size_t)cols, mbf, uR.data(), dK.data());

    // section 3: ORBmatcher
    int dist = orbm_descriptor_distance(desc.data(), desc.data() + 32);
    std::vector<Point2f> vbPrevMatched(n);
    std::vector<int> vnMatches12(n);
    const orbm_grid g{0.f, 0.f, 64.f / cols, 48.f / rows};
    int nmatches = 0, windowSize = 100, mbCheckOrientation = 1;
    float mfNNratio = 0.9f;
    orbm_search_for_initialization(0, (const orbx_keypoint*)kps.data(), desc.data(), n, (const orbx_keypoint*)kps.data(),
                                   desc.data(), n, &g, (float*)vbPrevMatched.data(), windowSize, mfNNratio,
                                   mbCheckOrientation, vnMatches12.data(), &nmatches);
    int nframes = 2, npairs = 1;
    const int *d_pair_a = nullptr, *d_pair_b = nullptr;
    float* d_prev = nullptr;
    int *d_m12 = nullptr, *d_nm = nullptr;
    orbm_search_for_initialization_device(d_kps, d_desc, d_counts, nframes, cap, d_pair_a, d_pair_b, npairs, &g, 100,
                                          0.9f, 1, d_prev, d_m12, d_nm, stream);
    orbm_search_init_batch_device(d_kps, d_desc, d_counts, nframes, cap, d_pair_a, d_pair_b, npairs, rows, cols, 100,
                                  0.9f, 1, d_m12, d_nm, stream);

    // Tracking::MonocularInitialization: Initializer::Initialize on the matches where they lie
    {
        orbm_pose_params Pi = {};
        const int* d_draws = nullptr;   // 8 * 200 rand() values per pair
        void* d_init_work = nullptr;    // hipMalloc once
        size_t init_bytes = orbm_init_workspace_bytes(npairs, cap, 200);
        orbm_init_out d_out = {};       // device arrays, one row per pair
        orbm_initialize_device(d_kps, d_counts, nframes, cap, d_pair_a, d_pair_b, npairs, d_m12, cap, d_draws, 8 * 200,
                               &Pi, 1.0f, 200, ORBM_INIT_PRUNE_MATCHES, d_init_work, init_bytes, &d_out, stream);
        // ... and one pair on host arrays
        std::vector<int> ini_matches(n, -1), pruned(n), draws(8 * 200), sets(8 * 200);
        for (int& r : draws) r = rand();
        std::vector<uint8_t> inlH(n), inlF(n), tri(n);
        std::vector<float> p3d(3 * n);
        int status = 0, model = 0, reason = 0, left = 0, ngood8[8];
        float scores[2], H21[9], F21[9], R21[9], t21[3], parallax8[8];
        orbm_init_out o = {&status, &model, &reason, scores, H21, F21, inlH.data(), inlF.data(), R21, t21,
                           p3d.data(), tri.data(), ngood8, parallax8, &left, pruned.data()};
        orbm_initialize(0, (const orbx_keypoint*)kps.data(), n, (const orbx_keypoint*)kps.data(), n, ini_matches.data(),
                        draws.data(), &Pi, 1.0f, 200, ORBM_INIT_PRUNE_MATCHES, &o);
        orbx_init_sets(n, draws.data(), 200, sets.data());
        if ((status & ORBM_INIT_FAILED) && reason == ORBM_INIT_H_TEST) left = 0;
    }

    // ComputeStereoMatches and its coarse stage
    std::vector<float> mvuRight(n, -1.f), mvDepth(n, -1.f), mvScaleFactors(8, 1.f);
    int ngood = 0;
    float minD = 0.f, maxD = 435.2f;
    orbx_compute_stereo_matches(hl, hr, (const orbx_keypoint*)kps.data(), desc.data(), n,
                                (const orbx_keypoint*)kps.data(), desc.data(), n, mbf, fx, mvuRight.data(),
                                mvDepth.data(), &ngood);
    std::vector<int> bestIdxR(n), bestDist(n);
    orbm_stereo_band(0, (const orbx_keypoint*)kps.data(), desc.data(), n, (const orbx_keypoint*)kps.data(), desc.data(),
                     n, rows, mvScaleFactors.data(), (int)mvScaleFactors.size(), minD, maxD, bestIdxR.data(),
                     bestDist.data());

    // orbm_best2_csr
    std::vector<int> cand_ptr(n + 1), cand_idx(1), best_idx(n), best(n), second(n);
    orbm_best2_csr(0, desc.data(), n, desc.data(), n, cand_ptr.data(), cand_idx.data(), ORBM_TIE_FIRST, best_idx.data(),
                   best.data(), second.data());

    // SearchByProjection(Frame&, vector<MapPoint*>, th)
    float th = 1.f;
    orbm_proj_params prm{0.f, 0.f, 64.f / cols, 48.f / rows, th, mfNNratio, {}};
    std::vector<orbm_proj_point> pts(10);
    std::vector<uint8_t> pdesc(10 * 32), claimed(n);
    std::vector<int> match(n);
    orbm_search_by_projection(0, (const orbx_keypoint*)kps.data(), desc.data(), mvuRight.data(), claimed.data(), n,
                              pts.data(), pdesc.data(), (int)pts.size(), &prm, match.data(), &nmatches);

    // the pose-projection searches
    orbm_pose_params P{fx, fx, 600.f, 180.f, mbf, mbf / fx, 0.f, (float)cols, 0.f, (float)rows, 64.f / cols,
                       48.f / rows, 0.18232f, 8, th, 0, 0, 1, {}, {}};
    std::vector<orbm_map_point> mps(10);
    std::vector<uint8_t> taken(n);
    float pose[24] = {};
    orbm_project_search(0, ORBM_PROJ_LAST_FRAME, (const orbx_keypoint*)kps.data(), desc.data(), mvuRight.data(),
                        taken.data(), n, pose, mps.data(), pdesc.data(), (int)mps.size(), &P, match.data(), &nmatches);

    // Tracking::SearchLocalPoints
    int np = (int)mps.size(), nToMatch = 0;
    orbm_frustum(0, mps.data(), np, pose, &P, 0.5f, pts.data(), &nToMatch);
    const orbm_map_point* d_mps = nullptr;
    const int* d_npts = nullptr;
    const float* d_Tcw = nullptr;
    const uint8_t *d_claimed = nullptr, *d_pdesc = nullptr;
    orbm_proj_point* d_pts = nullptr;
    int *d_ntomatch = nullptr, *d_match = nullptr, *d_nmatches = nullptr;
    int pcap = 4000;
    orbm_frustum_batch_device(d_mps, d_npts, nframes, pcap, d_Tcw, &P, 0.5f, d_pts, d_ntomatch, stream);
    orbm_search_by_projection_device(d_kps_un, d_desc, d_uright, d_claimed, d_counts, nframes, cap, d_pts, d_pdesc,
                                     d_npts, pcap, &prm, d_match, d_nmatches, stream);

    // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
    std::vector<uint8_t> mpdesc1(n * 32), mpdesc2(n * 32), already1(n), already2(n);
    std::vector<orbm_map_point> mps1(n), mps2(n);
    std::vector<int> match12(n);
    float T1w[12] = {}, T2w[12] = {}, s12 = 1.f, R12[9] = {}, t12[3] = {};
    int nFound = 0;
    P.th = 7.5f;
    orbm_search_by_sim3(0, (const orbx_keypoint*)kps.data(), desc.data(), mps1.data(), mpdesc1.data(), already1.data(),
                        n, T1w, (const orbx_keypoint*)kps.data(), desc.data(), mps2.data(), mpdesc2.data(),
                        already2.data(), n, T2w, s12, R12, t12, &P, match12.data(), &nFound, nullptr, nullptr);

    // MapPoint refresh: ComputeDistinctiveDescriptors + UpdateNormalAndDepth over a KeyFrame table
    int nkf = 3;
    std::vector<orbx_keypoint> tkps((size_t)nkf * cap);
    std::vector<uint8_t> tdesc((size_t)nkf * cap * 32), kf_bad(nkf);
    std::vector<int> tcounts(nkf), obs_ptr(np + 1), best_obs(np);
    std::vector<float> Tcw((size_t)nkf * 12);
    std::vector<orbm_observation> obs, ref(np);
    orbm_refresh_map_points(0, ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH, tkps.data(), tdesc.data(),
                            tcounts.data(), nkf, cap, Tcw.data(), kf_bad.data(), obs_ptr.data(), obs.data(), ref.data(),
                            np, &P, mps.data(), pdesc.data(), best_obs.data());
    const uint8_t* d_kf_bad = nullptr;
    const int* d_obs_ptr = nullptr;
    const orbm_observation *d_obs = nullptr, *d_ref = nullptr;
    orbm_map_point* d_mps_rw = nullptr;
    uint8_t* d_pdesc_rw = nullptr;
    int* d_best = nullptr;
    int max_obs = 64;
    orbm_refresh_map_points_device(ORBM_REFRESH_NORMAL_DEPTH, d_kps_un, d_desc, d_counts, nkf, cap, d_Tcw, d_kf_bad,
                                   d_obs_ptr, d_obs, d_ref, np, max_obs, &P, d_mps_rw, d_pdesc_rw, d_best, stream);

    // New MapPoints: the match loop of LocalMapping::CreateNewMapPoints, one neighbour on host arrays
    std::vector<float> uright(n, -1.0f), depth(n, -1.0f), x3d((size_t)3 * n);
    std::vector<int> vmatch(n, -1), tri_status(n), new_idx1(n);
    std::vector<orbm_map_point> new_pts(n);
    std::vector<orbm_observation> new_obs((size_t)2 * n), new_ref(n);
    std::vector<uint8_t> has_mp1(n), has_mp2(n);
    int nnew = 0;
    orbm_triangulate(0, (const orbx_keypoint*)kps.data(), (const orbx_keypoint*)kps.data(), uright.data(), depth.data(),
                     n, T1w, (const orbx_keypoint*)kps.data(), (const orbx_keypoint*)kps.data(), uright.data(),
                     depth.data(), n, T2w, vmatch.data(), &P, x3d.data(), tri_status.data(), new_pts.data(),
                     new_obs.data(), new_ref.data(), new_idx1.data(), &nnew, has_mp1.data(), has_mp2.data());
    if (nnew > 0 && tri_status[new_idx1[0]] == ORBM_TRI_CREATED_SVD) new_pts[0].flags = 3;
    // ... and any number of pairs on the device, emitting the refresh's d_pts / d_obs / d_ref
    const orbx_keypoint* d_kps_raw = nullptr;
    const float *d_uright_t = nullptr, *d_depth_t = nullptr;
    const int *d_rank = nullptr, *d_tri_a = nullptr, *d_tri_b = nullptr, *d_vmatch = nullptr;
    float* d_x3d = nullptr;
    int *d_tri_status = nullptr, *d_new_idx1 = nullptr, *d_nnew = nullptr;
    orbm_map_point* d_new_pts = nullptr;
    orbm_observation *d_new_obs = nullptr, *d_new_ref = nullptr;
    uint8_t* d_has_mp = nullptr;
    int tri_pairs = 20, match_stride = cap;
    orbm_triangulate_device(d_kps_un, d_kps_raw, d_uright_t, d_depth_t, d_counts, nkf, cap, d_Tcw, d_rank, d_tri_a,
                            d_tri_b, tri_pairs, d_vmatch, match_stride, &P, d_x3d, d_tri_status, d_new_pts, d_new_obs,
                            d_new_ref, d_new_idx1, d_nnew, d_has_mp, stream);
    orbm_refresh_map_points_device(ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH, d_kps_un, d_desc, d_counts, nkf,
                                   cap, d_Tcw, d_kf_bad, d_obs_ptr, d_new_obs, d_new_ref, match_stride, 2, &P,
                                   d_new_pts, d_pdesc_rw, d_best, stream);

    // Tracking::TrackLocalMap: UpdateLocalMap -> isInFrustum -> SearchByProjection on one stream
    const int *d_kf_mp = nullptr, *d_covis = nullptr, *d_child_ptr = nullptr, *d_child = nullptr, *d_parent = nullptr;
    const int *d_fcounts = nullptr, *d_frame_outlier = nullptr;
    int *d_frame_mp = nullptr, *d_local_kf = nullptr, *d_nlocal_kf = nullptr, *d_ref_kf = nullptr;
    int *d_local_mp = nullptr, *d_nlocal = nullptr, *d_lm_status = nullptr;
    orbm_map_point* d_local_pts = nullptr;
    uint8_t *d_local_pdesc = nullptr, *d_local_claimed = nullptr;
    void* d_work = nullptr;   // hipMalloc + hipMemset once; every call leaves it zeroed
    int nmp = 100000, kfcap = 96;
    size_t work_bytes = orbm_local_map_work_bytes(nkf, nmp, nframes, kfcap);
    orbm_local_map_device(d_counts, d_kf_mp, d_kf_bad, d_rank, d_covis, d_child_ptr, d_child, d_parent, nkf, cap,
                          d_mps_rw, d_pdesc_rw, d_obs_ptr, d_obs, nmp, d_fcounts, d_frame_mp, d_frame_outlier, nframes,
                          cap, d_local_kf, d_nlocal_kf, kfcap, d_ref_kf, d_local_mp, d_nlocal, d_local_pts,
                          d_local_pdesc, pcap, d_local_claimed, d_lm_status, d_work, work_bytes, stream);
    orbm_frustum_batch_device(d_local_pts, d_nlocal, nframes, pcap, d_Tcw, &P, 0.5f, d_pts, d_ntomatch, stream);
    orbm_search_by_projection_device(d_kps_un, d_desc, d_uright, d_local_claimed, d_fcounts, nframes, cap, d_pts,
                                     d_local_pdesc, d_nlocal, pcap, &prm, d_match, d_nmatches, stream);
    // Tracking::Track with the pose on the device: Optimizer::PoseOptimization in its three places.  d_Tcw_rw holds
    // the frame's mTcw and is handed to the next frustum test / search as it is; d_outl is mvbOutlier.
    float* d_Tcw_rw = nullptr;
    float* d_Tcw_opt = nullptr;   // the optimised pose: may not alias the input
    uint8_t* d_outl = nullptr;
    int *d_frame_outlier_rw = nullptr, *d_ninliers = nullptr, *d_nmatches_map = nullptr, *d_po_status = nullptr;
    orbm_pose_opt_trace* d_po_trace = nullptr;   // or NULL
    // TrackReferenceKeyFrame (:827) / TrackWithMotionModel (:950): after SearchByBoW / SearchByProjection wrote
    // d_frame_mp; the discard loop (:830-848, :953-972) runs inside the call
    orbm_pose_optimization_device(d_kps_un, d_uright, d_fcounts, nframes, cap, d_frame_mp, d_mps_rw, nmp, d_Tcw_rw, 12,
                                  &P, ORBM_POSE_OPT_DISCARD, d_Tcw_opt, d_outl, d_frame_outlier_rw, d_ninliers,
                                  d_nmatches_map, d_po_trace, d_po_status, stream);
    // TrackLocalMap: UpdateLocalMap takes the discarded outliers, the frustum test and the search the new pose ...
    orbm_local_map_device(d_counts, d_kf_mp, d_kf_bad, d_rank, d_covis, d_child_ptr, d_child, d_parent, nkf, cap,
                          d_mps_rw, d_pdesc_rw, d_obs_ptr, d_obs, nmp, d_fcounts, d_frame_mp, d_frame_outlier_rw,
                          nframes, cap, d_local_kf, d_nlocal_kf, kfcap, d_ref_kf, d_local_mp, d_nlocal, d_local_pts,
                          d_local_pdesc, pcap, d_local_claimed, d_lm_status, d_work, work_bytes, stream);
    orbm_frustum_batch_device(d_local_pts, d_nlocal, nframes, pcap, d_Tcw_opt, &P, 0.5f, d_pts, d_ntomatch, stream);
    orbm_search_by_projection_device(d_kps_un, d_desc, d_uright, d_local_claimed, d_fcounts, nframes, cap, d_pts,
                                     d_local_pdesc, d_nlocal, pcap, &prm, d_match, d_nmatches, stream);
    // ... and the third optimisation (:992): no discard, d_nmatches_map = mnMatchesInliers
    orbm_pose_optimization_device(d_kps_un, d_uright, d_fcounts, nframes, cap, d_frame_mp, d_mps_rw, nmp, d_Tcw_opt, 12,
                                  &P, 0, d_Tcw_rw, d_outl, nullptr, d_ninliers, d_nmatches_map, nullptr, d_po_status,
                                  stream);
    // Relocalization (:1492-1523): one candidate on host arrays, up to three times around the projection searches
    {
        std::vector<int> fmp(n, -1), fout(n, -1);
        std::vector<uint8_t> outl(n, 0);
        float Tcw_in[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, Tcw_out[12];
        int nGood = 0, nMap = 0, po_status = 0;
        orbm_pose_opt_trace po_trace;
        orbm_pose_optimization(0, (const orbx_keypoint*)kps.data(), uright.data(), n, fmp.data(), mps.data(), np, Tcw_in,
                               &P, 0, Tcw_out,
                               outl.data(), fout.data(), &nGood, &nMap, &po_trace, &po_status);
        if (po_status & ORBM_POSE_OPT_INVALID) nGood = 0;
    }
    // ... and one frame on host arrays
    std::vector<int> kf_mp((size_t)nkf * cap, -1), kf_covis((size_t)nkf * 10, -1), child_ptr(nkf + 1), child;
    std::vector<int> parent(nkf, -1), frame_mp(n, -1), local_kf(kfcap), local_mp(pcap);
    std::vector<orbm_map_point> local_pts(pcap);
    std::vector<uint8_t> local_pdesc((size_t)pcap * 32), local_claimed(n);
    int nlocal_kf = 0, ref_kf = -1, nlocal = 0, lm_status = 0;
    orbm_local_map(0, tcounts.data(), kf_mp.data(), kf_bad.data(), nullptr, kf_covis.data(), child_ptr.data(),
                   child.data(), parent.data(), nkf, cap, mps.data(), pdesc.data(), obs_ptr.data(), obs.data(), np, n,
                   frame_mp.data(), nullptr, local_kf.data(), &nlocal_kf, kfcap, &ref_kf, local_mp.data(), &nlocal,
                   local_pts.data(), local_pdesc.data(), pcap, local_claimed.data(), &lm_status);
    if (lm_status & ORBM_LOCAL_MAP_INVALID) nlocal = 0;

    // the covisibility graph: KeyFrame::UpdateConnections after an insertion, then the tables the calls above take
    int ccap = 256, new_kf = nkf - 1, root = 0, ntargets = 1;
    orbm_covis_graph graph{};   // eight hipMalloc'ed arrays: nkf * ccap rows, nkf counts, parent, first (memset to 1)
    int *d_targets = nullptr, *d_conn_status = nullptr, *d_covis_rw = nullptr, *d_child_ptr_rw = nullptr;
    int *d_child_rw = nullptr, *d_child_status = nullptr, *d_by_weight = nullptr;
    uint8_t* d_connected = nullptr;
    void *d_conn_work = nullptr, *d_child_work = nullptr;   // hipMalloc + hipMemset once each
    size_t conn_bytes = orbm_connections_work_bytes(nkf, ccap), child_bytes = orbm_children_work_bytes(nkf);
    orbm_update_connections_device(&graph, nkf, ccap, d_counts, d_kf_mp, cap, d_rank, d_mps_rw, d_obs_ptr, d_obs, nmp,
                                   d_targets, ntargets, /*th*/ 15, root, d_conn_status, d_conn_work, conn_bytes,
                                   stream);
    orbm_best_covisibles_device(&graph, nkf, ccap, 10, d_covis_rw, stream);          // d_covis
    orbm_children_device(graph.parent, d_kf_bad, d_rank, nkf, d_child_ptr_rw, d_child_rw, d_child_status,
                         d_child_work, child_bytes, stream);                          // d_child_ptr, d_child
    orbm_connected_mask_device(&graph, nkf, ccap, new_kf, d_connected, stream);      // DetectLoopCandidates
    orbm_covisibles_by_weight_device(&graph, nkf, ccap, 100, d_by_weight, stream);   // the essential graph
    // KeyFrame::SetBadFlag's connection part
    orbm_erase_connections_device(&graph, nkf, ccap, d_rank, d_targets, ntargets, d_conn_status, d_conn_work,
                                  conn_bytes, stream);
    // ... and on host arrays
    std::vector<int> conn_kf((size_t)nkf * ccap), conn_w((size_t)nkf * ccap), ord_kf((size_t)nkf * ccap);
    std::vector<int> ord_w((size_t)nkf * ccap), nconn(nkf), nord(nkf), conn_status(ntargets);
    std::vector<uint8_t> first(nkf, 1);
    orbm_covis_graph hgraph{conn_kf.data(), conn_w.data(), nconn.data(), ord_kf.data(), ord_w.data(), nord.data(),
                            parent.data(), first.data()};
    orbm_update_connections(0, &hgraph, nkf, ccap, tcounts.data(), kf_mp.data(), cap, nullptr, mps.data(),
                            obs_ptr.data(), obs.data(), np, &new_kf, ntargets, 15, root, conn_status.data());
    if (conn_status[0] == ORBM_CONN_NOSPC || conn_status[0] == ORBM_CONN_INVALID) nlocal = 0;

    // LocalMapping::Run: MapPointCulling ... KeyFrameCulling, then the compaction and the culled KeyFrames' connections
    int *d_kf_mp_rw = nullptr, *d_recent = nullptr, *d_recent_out = nullptr, *d_nrecent_out = nullptr;
    int *d_nobs = nullptr, *d_found = nullptr, *d_visible = nullptr, *d_first_kfid = nullptr, *d_mp_verdict = nullptr;
    int *d_kf_verdict = nullptr, *d_nmps = nullptr, *d_nred = nullptr, *d_culled = nullptr, *d_nculled = nullptr;
    int *d_ncull_cand = nullptr, *d_obs_ptr_out = nullptr, *d_compact_status = nullptr, *d_erase_status = nullptr;
    uint8_t *d_obs_erased = nullptr, *d_kf_noterase = nullptr;
    orbm_observation *d_ref_rw = nullptr, *d_obs_out = nullptr;
    void* d_cull_work = nullptr;   // hipMalloc + hipMemset once
    int nrecent = 500, cur_kfid = 321;
    size_t cull_bytes = orbm_culling_work_bytes(nmp);
    orbm_map_point_culling_device(d_recent, nrecent, cur_kfid, /*nThObs*/ 3, d_counts, d_kf_mp_rw, nkf, cap, d_mps_rw,
                                  d_obs_ptr, d_obs, d_obs_erased, nmp, d_nobs, d_found, d_visible, d_first_kfid,
                                  d_mp_verdict, d_recent_out, d_nrecent_out, stream);
    orbm_keyframe_culling_device(&graph, nkf, ccap, new_kf, root, d_counts, d_kf_mp_rw, cap, d_kps_un, d_uright_t,
                                 d_depth_t, /*mThDepth*/ 35.0f, /*!mbMonocular*/ 1, P.nlevels, d_kf_noterase, d_mps_rw,
                                 d_obs_ptr, d_obs, d_obs_erased, d_ref_rw, d_nobs, nmp, d_kf_verdict, d_nmps, d_nred,
                                 d_culled, d_nculled, d_ncull_cand, d_cull_work, cull_bytes, stream);
    orbm_compact_observations_device(d_obs_ptr, d_obs, d_obs_erased, nmp, d_obs_ptr_out, d_obs_out, d_compact_status,
                                     stream);
    orbm_erase_connections_device(&graph, nkf, ccap, d_rank, d_culled, ccap, d_erase_status, d_conn_work, conn_bytes,
                                  stream);
    // ... and on host arrays
    std::vector<int> recent(nrecent), recent_out(nrecent), mp_verdict(nrecent), nobs(np), found(np), visible(np);
    std::vector<int> first_kfid(np), kf_verdict(ccap), nmps(ccap), nred(ccap), culled(ccap), obs_ptr_out(np + 1);
    std::vector<uint8_t> obs_erased(obs.size()), kf_noterase(nkf);
    std::vector<orbm_observation> cull_ref(np), obs_out(obs.size());
    std::vector<float> kf_uright((size_t)nkf * cap, -1.0f), kf_depth((size_t)nkf * cap, -1.0f);
    std::vector<orbx_keypoint> kf_kps((size_t)nkf * cap);
    int nrecent_out = 0, nculled = 0, ncands = 0, compact_status = 0;
    orbm_map_point_culling(0, recent.data(), nrecent, cur_kfid, 3, tcounts.data(), kf_mp.data(), nkf, cap, mps.data(),
                           obs_ptr.data(), obs.data(), obs_erased.data(), np, nobs.data(), found.data(),
                           visible.data(), first_kfid.data(), mp_verdict.data(), recent_out.data(), &nrecent_out);
    orbm_keyframe_culling(0, &hgraph, nkf, ccap, new_kf, root, tcounts.data(), kf_mp.data(), cap, kf_kps.data(),
                          kf_uright.data(), kf_depth.data(), 35.0f, 1, P.nlevels, kf_noterase.data(), mps.data(),
                          obs_ptr.data(), obs.data(), obs_erased.data(), cull_ref.data(), nobs.data(), np, kf_verdict.data(),
                          nmps.data(), nred.data(), culled.data(), &nculled, &ncands);
    orbm_compact_observations(0, obs_ptr.data(), obs.data(), obs_erased.data(), np, obs_ptr_out.data(), obs_out.data(),
                              &compact_status);
    if (mp_verdict[0] == ORBM_CULL_INVALID || kf_verdict[0] == ORBM_KFCULL_INVALID) nlocal = 0;

    // LoopClosing::ComputeSim3: SearchByBoW(KF, KF) -> Sim3Solver -> SearchBySim3 on one stream
    const orbm_bow_view *d_view_cur = nullptr, *d_view_cand = nullptr;   // one row per candidate
    const int *d_cand_a = nullptr, *d_cand_b = nullptr, *d_rand = nullptr, *d_rand_off = nullptr;
    const uint8_t* d_mpdesc = nullptr;
    int ncands3 = 8, max_nodes1 = 1000;
    int *d_bow12 = nullptr, *d_nbow = nullptr, *d_s3_n = nullptr, *d_s3_its = nullptr, *d_s3_best = nullptr;
    int *d_s3_status = nullptr, *d_s3_ninl = nullptr, *d_s3_nomore = nullptr, *d_s3_used = nullptr;
    int *d_s3_match12 = nullptr, *d_s3_nfound = nullptr;
    float* d_sim3 = nullptr;
    uint8_t *d_inliers12 = nullptr, *d_already2 = nullptr;
    std::vector<int> maxits((size_t)cap + 1);   // mRansacMaxIts per N, once per parameter set; copied to d_maxits
    for (int k = 0; k <= cap; k++) maxits[k] = orbm_sim3_ransac_iterations(k, 0.99, 20, 300);
    const int* d_maxits = nullptr;
    size_t s3_bytes = orbm_sim3_workspace_bytes(ncands3, cap, 5);
    void* d_s3_work = nullptr;   // hipMalloc once
    orbm_bow_search_device(ORBM_BOW_KF_KF, d_view_cur, d_view_cand, nullptr, ncands3, max_nodes1, 0.75f, 1, d_bow12, cap,
                           d_nbow, stream);
    orbm_sim3_setup_device(d_kps_un, d_counts, nkf, cap, d_Tcw, d_kf_mp, d_mps_rw, nmp, d_obs_ptr, d_obs, d_obs_erased,
                           d_cand_a, d_cand_b, ncands3, d_bow12, cap, &P, d_maxits, d_s3_work, s3_bytes, d_s3_n,
                           d_s3_its, d_s3_best, d_s3_status, stream);
    // one round of the while loop (:286-342): five iterations of every candidate still in play
    orbm_sim3_iterate_device(d_s3_work, s3_bytes, ncands3, cap, &P, /*mbFixScale*/ 0, 20, 5, d_rand, d_rand_off,
                             d_s3_its, d_s3_best, d_sim3, d_inliers12, d_already2, d_s3_ninl, d_s3_nomore, d_s3_used,
                             stream);
    orbm_search_by_sim3_device(d_kps_un, d_desc, d_mps_rw, d_mpdesc, d_counts, nkf, cap, d_Tcw, d_cand_a, d_cand_b,
                               d_sim3, d_inliers12, d_already2, ncands3, &P, d_s3_match12, d_s3_nfound, nullptr,
                               nullptr, stream);
    // ... and one candidate on host arrays: a new solver's first five iterations
    {
        std::vector<int> mp1(n, -1), mp2(n, -1), bow12(n, -1), draws(15);
        std::vector<uint8_t> inl12(n), alr2(n);
        for (int& r : draws) r = rand();
        int its = 0, best = 0, N = 0, nInliers = 0, bNoMore = 0, used = 0, s3_status = 0;
        float sim3[13];
        orbm_sim3_solve(0, (const orbx_keypoint*)kps.data(), mp1.data(), n, T1w, (const orbx_keypoint*)kps.data(),
                        mp2.data(), n, T2w, mps.data(), np, obs_ptr.data(), obs.data(), obs_erased.data(), bow12.data(),
                        &P, 0, 0.99, 20, 300, 5, draws.data(), &its, &best, &N, sim3, inl12.data(), alr2.data(),
                        &nInliers, &bNoMore, &used, &s3_status);
        if (s3_status & ORBM_SIM3_INVALID) nInliers = 0;
    }
    // ... -> the gather -> OptimizeSim3, whose d_scw SearchByProjection(pKF, Scw, ...) reads
    int *d_matches1 = nullptr, *d_os_nin = nullptr, *d_os_status = nullptr;
    double* d_g2o_sim3 = nullptr;
    float *d_sim3_opt = nullptr, *d_scw = nullptr;
    orbm_opt_sim3_trace* d_os_trace = nullptr;
    orbm_sim3_gather_matches_device(d_kf_mp, d_counts, nkf, cap, d_cand_a, d_cand_b, ncands3, d_inliers12, d_bow12, cap,
                                    d_s3_match12, d_matches1, cap, stream);
    orbm_optimize_sim3_device(d_kps_un, d_counts, nkf, cap, d_Tcw, d_kf_mp, d_mps_rw, nmp, d_obs_ptr, d_obs,
                              d_obs_erased, d_cand_a, d_cand_b, ncands3, d_sim3, d_matches1, cap, 10.0f,
                              /*mbFixScale*/ 0, &P, d_g2o_sim3, d_sim3_opt, d_scw, d_os_nin, d_os_trace, d_os_status,
                              stream);
    {
        std::vector<int> mp1(n, -1), matches1(n, -1);
        float sim3[13] = {1.0f, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, sim3_opt[13], Scw[12];
        double g2oS12[8];
        int nInliers = 0, os_status = 0;
        orbm_optimize_sim3(0, (const orbx_keypoint*)kps.data(), mp1.data(), n, T1w, (const orbx_keypoint*)kps.data(), n,
                           T2w, mps.data(), np, obs_ptr.data(), obs.data(), obs_erased.data(), sim3, matches1.data(),
                           10.0f, 0, &P, g2oS12, sim3_opt, Scw, &nInliers, nullptr, &os_status);
        if (os_status & ORBM_OPT_SIM3_INVALID) nInliers = 0;
    }

    // Tracking::Relocalization: SearchByBoW(KF, F) -> PnPsolver -> PoseOptimization on one stream
    const orbm_bow_view *d_view_kf = nullptr, *d_view_f = nullptr;   // one row per candidate KeyFrame
    const int *d_frame_of = nullptr, *d_kf_of = nullptr, *d_pnp_rand = nullptr, *d_pnp_rand_off = nullptr;
    int ncands_pnp = 8, nrand = 8 * 4 * 300;
    int *d_bow_f = nullptr, *d_nbow_f = nullptr, *d_pnp_n = nullptr, *d_pnp_its = nullptr, *d_pnp_best = nullptr;
    int *d_pnp_status = nullptr, *d_pnp_has = nullptr, *d_pnp_ninl = nullptr, *d_pnp_nomore = nullptr;
    int *d_pnp_used = nullptr, *d_pnp_frame_mp = nullptr;
    float* d_pnp_tcw = nullptr;
    uint8_t* d_pnp_inliers = nullptr;
    // mRansacMinInliers and mRansacMaxIts per N, once per parameter set; copied to d_pnp_mininl / d_pnp_maxits
    std::vector<int> pnp_mininl((size_t)cap + 1), pnp_maxits((size_t)cap + 1);
    for (int k = 0; k <= cap; k++)
        orbm_pnp_ransac_parameters(k, 0.99, 10, 300, 4, 0.5f, &pnp_mininl[k], &pnp_maxits[k]);
    const int *d_pnp_mininl = nullptr, *d_pnp_maxits = nullptr;
    size_t pnp_bytes = orbm_pnp_workspace_bytes(ncands_pnp, cap, 300);
    void* d_pnp_work = nullptr;   // hipMalloc once
    orbm_bow_search_device(ORBM_BOW_KF_F, d_view_kf, d_view_f, nullptr, ncands_pnp, max_nodes1, 0.75f, 1, d_bow_f, cap,
                           d_nbow_f, stream);
    orbm_pnp_setup_device(d_kps_un, d_counts, nkf, cap, d_kf_mp, nkf, d_mps_rw, nmp, d_frame_of, d_kf_of, ncands_pnp,
                          d_bow_f, cap, &P, 5.991f, d_pnp_mininl, d_pnp_maxits, 300, d_pnp_work, pnp_bytes, d_pnp_n,
                          d_pnp_its, d_pnp_best, d_pnp_status, stream);
    // one round of the while loop (:1456-1552): iterate(5) of every candidate still in play
    orbm_pnp_iterate_device(d_pnp_work, pnp_bytes, ncands_pnp, cap, &P, 4, 300, 5, d_pnp_rand, nrand, d_pnp_rand_off,
                            d_pnp_its, d_pnp_best, d_pnp_tcw, d_pnp_has, d_pnp_inliers, d_pnp_ninl, d_pnp_nomore,
                            d_pnp_used, d_pnp_frame_mp, stream);
    // ... and one candidate on host arrays: a new solver's first call
    {
        std::vector<int> kfmp(n, -1), bowf(n, -1), draws(4 * 300), fmp(n, -1);
        std::vector<uint8_t> inl(n);
        std::vector<uint64_t> pnp_state((orbm_pnp_state_bytes(n) + 7) / 8);
        for (int& r : draws) r = rand();
        int its = 0, best = 0, N = 0, has_pose = 0, nInliers = 0, bNoMore = 0, used = 0, pnp_status = 0;
        float Tcw[12];
        orbm_pnp_solve(0, (const orbx_keypoint*)kps.data(), n, kfmp.data(), n, mps.data(), np, bowf.data(), &P, 5.991f,
                       0.99, 10, 300, 4, 0.5f, 5, draws.data(), &its, &best, pnp_state.data(), &N, Tcw, &has_pose,
                       inl.data(), &nInliers, &bNoMore, &used, fmp.data(), &pnp_status);
        if (pnp_status & ORBM_PNP_INVALID) nInliers = 0;
    }

    // ComputeBoW
    std::vector<int32_t> bw(n), node(n), ptr(n + 1), idx(n);
    std::vector<double> bv(n);
    int nb = 0, nn = 0;
    orbv_transform(vocab_handle, desc.data(), n, 4, bw.data(), bv.data(), &nb, node.data(), ptr.data(), idx.data(),
                   &nn);

    // KeyFrameDatabase: add / erase / DetectLoop's reference scores / DetectLoopCandidates / DetectRelocalizationCandidates
    orbv_database* db = nullptr;
    orbv_db_create(vocab_handle, 0, 0, &db);
    int slot = -1, nslots = 0, nlive = 0, ncand = 0;
    size_t stored = 0;
    orbv_db_add(db, bw.data(), bv.data(), nb, &slot);
    orbv_db_info(db, &nslots, &nlive, &stored);
    std::vector<uint8_t> connected(nslots);
    std::vector<int32_t> covis(nslots * 10, -1);
    std::vector<int> cand(nslots), slots(nslots), words(nslots);
    std::vector<double> ref_scores(nslots);
    std::vector<float> kf_scores(nslots);
    double s12score = 0.0;
    orbv_score(0, bw.data(), bv.data(), nb, bw.data(), bv.data(), nb, &s12score);
    orbv_db_scores(db, bw.data(), bv.data(), nb, slots.data(), nslots, ref_scores.data());
    orbv_db_detect_loop(db, bw.data(), bv.data(), nb, connected.data(), covis.data(), (float)ref_scores[0], cand.data(),
                        nslots, &ncand, words.data(), kf_scores.data());
    orbv_db_detect_reloc(db, bw.data(), bv.data(), nb, covis.data(), cand.data(), nslots, &ncand, nullptr, nullptr);
    // replay: the BowVectors of a transform batch and its queries stay on the device
    int32_t* d_bw = nullptr; double* d_bv = nullptr; int* d_bn = nullptr; int* d_cand = nullptr; int* d_ncand = nullptr;
    orbv_db_add_batch_device(db, d_bw, d_bv, d_bn, 1, n, slots.data(), stream);
    orbv_db_detect_loop_device(db, d_bw, d_bv, d_bn, n, nullptr, nullptr, 0.05f, nslots + 1, d_cand, d_ncand, nullptr,
                               nullptr, stream);
    orbv_db_detect_reloc_device(db, d_bw, d_bv, d_bn, n, nullptr, nslots + 1, d_cand, d_ncand, nullptr, nullptr, stream);
    orbv_db_erase(db, slot);
    orbv_db_clear(db);
    orbv_db_destroy(db);

    // SearchByBoW(KeyFrame*, Frame&)
    std::vector<uint8_t> hasmp(n);
    std::vector<int> n1(1), p1(2), i1(1);
    orbm_bow_view a{(const orbx_keypoint*)kps.data(), desc.data(), hasmp.data(), nullptr, n1.data(), p1.data(),
                    i1.data(), n, (int)n1.size()};
    orbm_bow_view b{(const orbx_keypoint*)kps.data(), desc.data(), nullptr, nullptr, n1.data(), p1.data(), i1.data(),
                    n, (int)n1.size()};
    orbm_bow_search(0, ORBM_BOW_KF_F, &a, &b, nullptr, mfNNratio, mbCheckOrientation, match.data(), &nmatches);
    return dist + nmatches + ngood + nb + nn + nFound + ncand;
}

}  // namespace

int (*volatile orbx_abi_snippets)(orbx_handle*, orbx_handle*, orbx_handle*, orbx_vocabulary*, void*) = snippets;
