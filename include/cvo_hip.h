/* ============================================================================
 * include/cvo_hip.h -- C ABI of libcvo_hip.so: the MI355X (gfx950) implementation
 * of CVO-SLAM's per-frame-pair CVO alignment hot path.
 *
 * The reference has no FFI layer: the C++ class `cvo::cvo`
 * (thirdparty/cvo/include/cvo.hpp:82-282) IS the boundary that local_tracker /
 * keyframe_graph link against.  Each entry point below replaces one member of
 * that class (cited per function); a header-only `cvo::cvo` adaptor with the
 * reference's exact signatures forwards to them.  A point cloud
 * enters either as plain arrays (cvo_set_pcd: the reference's pcd_generator stays
 * on the host side of the adaptor) or as the RGB and depth images themselves
 * (cvo_set_pcd_images: the generator runs on the GPU, the cloud never leaves HBM).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are HOST pointers unless the
 *     name says `_device`.
 *   - point cloud = n x 3 f32 positions, AoS, 12-byte stride (cloud_t,
 *     data_type.h:30) + 5 channel-major f32 arrays of n (the column-major
 *     Eigen::Matrix<float,Dynamic,5> `features`, data_type.h:75).
 *   - rigid transforms = 3x4 row-major [R | t] (top rows of Eigen::Affine3f).
 *   - every call returns a status; the reference's functions are `void` and
 *     print-and-return on "not initialized" (cvo.cpp:463-466), which the adaptor
 *     reproduces from CVO_ERR_NOT_INITIALIZED.
 *   - a handle is used by one thread at a time; distinct handles are independent
 *     (own HIP stream, no globals), like distinct cvo::cvo objects.
 * ========================================================================== */
#ifndef CVO_HIP_H
#define CVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CVO_OK = 0,
    CVO_ERR_NOT_INITIALIZED = 1,  /* cvo.cpp:463-466 / 565-568 */
    CVO_ERR_EMPTY_CLOUD = 2,      /* reference: KD adaptor assert / UB (Q8) */
    CVO_ERR_HIP = 3,              /* HIP runtime error, message via cvo_last_error() */
    CVO_ERR_INVALID = 4,          /* bad argument */
    CVO_ERR_NO_DEVICE = 5,        /* no gfx950 device: the library never falls back to the CPU */
    CVO_ERR_TIMEOUT = 6,          /* in-kernel inter-workgroup wait gave up */
    CVO_ERR_PADDING = 7,          /* status field of a gathered result record that stands for no pair (shard padding); never returned by a call */
    CVO_ERR_RANK_FAILED = 8       /* status field of the records a rank contributes to a gather when it could not prepare its own block (the rank's
                                     call returned the cause); never returned by a call */
};

enum { CVO_SLOT_FIXED = 0, CVO_SLOT_MOVING = 1, CVO_SLOT_PREVIOUS = 2 };   /* cvo.hpp:91-94 */

/* Hyper-parameters the reference hard-codes in the ctor (cvo.cpp:35-51). */
typedef struct cvo_params {
    float ell;        /* 0.15  initial kernel length-scale        cvo.cpp:35 */
    float sigma;      /* 0.1                                      cvo.cpp:36 */
    float sp_thres;   /* 8e-3  sparsification threshold           cvo.cpp:37 */
    float c;          /* 7.0   so(3) inner-product scale          cvo.cpp:38 */
    float d;          /* 7.0   R^3 inner-product scale            cvo.cpp:39 */
    float c_ell;      /* 200   colour kernel length-scale         cvo.cpp:41 */
    float c_sigma;    /* 1                                        cvo.cpp:42 */
    int   max_iter;   /* 2000                                     cvo.cpp:48 */
    float min_step;   /* 0.2                                      cvo.cpp:49 */
    float eps;        /* 5e-5  stop A                             cvo.cpp:50 */
    float eps_2;      /* 1e-5  stop B                             cvo.cpp:51 */
} cvo_params;

/* inn_p, cvo.hpp:52-80 */
typedef struct cvo_inn_p { float value; int num; int num_e; } cvo_inn_p;

/* one align() iteration as the kernel saw it (parity/diagnostics; optional) */
typedef struct cvo_trace_row {
    float  omega[3];
    float  v[3];
    int    nnz;
    int    candidates;   /* pairs that passed the conservative cull (>= nnz) */
    double B, C, D, E;
    float  step;
    float  ell;
    float  dist;         /* dist_se3 of the applied update, -1 if stop A fired first */
    int    pad_;
} cvo_trace_row;

typedef struct cvo_handle_s* cvo_handle;

const char* cvo_last_error(void);                 /* thread-local message of the last failing call */
int cvo_device_count(void);                       /* number of visible gfx950 devices */
int cvo_default_params(cvo_params* p);            /* ctor constants, cvo.cpp:35-51 */

/* ---- object lifetime:  cvo::cvo(const string& calib_file) / ~cvo()  cvo.cpp:18-74
 * (the calib file only feeds pcd_generator, which stays on the adaptor side) */
int cvo_create(const cvo_params* p /* NULL = defaults */, int device, cvo_handle* out);
int cvo_destroy(cvo_handle h);

/* ---- set_pcd(RGB, depth)  cvo.cpp:345-386, with the selected cloud handed in.
 * First call fills FIXED and sets `init`; later calls replace MOVING. */
int cvo_set_pcd(cvo_handle h, const float* xyz, const float* feat, int n);

/* ---- align()  cvo.cpp:763-821.  Runs entirely on the device from the handle's
 * R, T, ell (warm start, Q1/Q2) and leaves R, T, ell, transform, iter, A_nonzero
 * updated.  trace may be NULL. */
int cvo_align(cvo_handle h);
int cvo_align_traced(cvo_handle h, cvo_trace_row* trace, int trace_cap, int* trace_len);

/* ---- set_pcd(RGB_img, dep_img) with the reference's pcd_generator on the GPU  cvo.cpp:345-386
 * (SURVEY 8f next-1): gray image, 3-level gradient pyramid (pcd_generator.cpp:50-143), DSO pixel selection
 * (thirdparty/PixelSelector2.cpp:34-436, num_want points, srand(3141592) sub-sampling pattern), back-projection
 * and (B,G,R,dx,dy) features (pcd_generator.cpp:456-499, 590-612), written straight into the HBM cloud the
 * alignment reads.  bgr8: height x width x 3 bytes (cv::Mat CV_8UC3, row stride 3*width); depth16: height x
 * width uint16 (0 = invalid); cam = cvo::camera_info (data_type.h:33-39, read from the calib file by the ctor).
 * Same slot semantics as cvo_set_pcd.
 * The tracker hands one frame to two objects (cvo_odometry->match_odometry(frame), cvo_keyframe->match_keyframe(frame), local_tracker.cpp:356, 415) and the
 * selector is deterministic, so the two MOVING clouds are the same cloud: a handle that is given, on the same host thread and device, byte for byte the images
 * (and camera, num_want) the thread's previous generation was given takes a device copy of that cloud instead of generating it again (the staged images are kept
 * for the compare; a different frame differs within its first bytes).  Same bits either way (tests/test_gpu_pcd.py); CVO_HIP_SHARE_CLOUDS=0 generates always.
 * cvo_shared_cloud_count: how many of this handle's clouds were taken that way. */
typedef struct cvo_camera { float scaling_factor, fx, fy, cx, cy; } cvo_camera;
int cvo_set_pcd_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height,
                       const cvo_camera* cam);
int cvo_shared_cloud_count(cvo_handle h, int* count);
/* Start the generation of a frame's cloud AHEAD of the cvo_set_pcd_images that will ask for it.  The reference handles a frame strictly in sequence
 * (local_tracker.cpp:356 -> 375 -> 407 -> 415 -> 431) and every frame starts by waiting for its generator (cvo.cpp:348-366); frame t + 1's images do not depend on
 * frame t's alignments, so a caller that has them (run_SLAM.cpp:70-87 loads the next image right after this one) hands them over here, e.g. between the odometry
 * block and the keyframe block of frame t, and goes on: a worker thread with a stream and scratch of its own runs the generator beside frame t's keyframe
 * alignment (eight workgroups of 256 compute units), and frame t + 1's cvo_set_pcd_images -- on this host thread and device, given byte for byte these images,
 * this camera and the handle's num_want -- takes the finished cloud (waiting for it if need be; then the frame's second object takes its copy as it always did).
 * Returns at once.  The two images must stay valid and unchanged until that cvo_set_pcd_images (or the next cvo_stage_next_frame) has returned; one frame is
 * staged per host thread, a frame never asked for is dropped.  Nothing changes in what any call computes: same cloud bits (tests/test_gpu_pcd.py).
 * cvo_staged_frame_count: how many of this handle's clouds were taken from a staged generation. */
int cvo_stage_next_frame(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera* cam);
int cvo_staged_frame_count(cvo_handle h, int* count);
/* The tracker calls compute_innerproduct(tran = the transform match_* has just returned) behind every alignment (local_tracker.cpp:356-375, 415-431;
 * cvo.cpp:475-503).  An alignment of this handle can start that score block itself -- the score kernel is queued behind the align kernel with the transform
 * and ell taken from the pair's device-resident state, cvo_align returns as soon as the alignment is in, and cvo_compute_innerproduct only collects when it is
 * asked for exactly that transform on the same clouds at the same ell; any other request runs the score kernel as before.  Same numbers either way
 * (tests/test_gpu_tail_scores.py).  on = 0: never; 1: every alignment; 2 (the default): an alignment does when the handle's PREVIOUS alignment was followed by
 * exactly that question -- the tracker's two objects from their second frame on, a loop-closure object (cvo_compute_innerproduct_lc) never, and an alignment nobody
 * scores queues nothing after the first miss.  CVO_HIP_HANDLE_TAIL=kernel: the batches' way instead (the align launch's own tail, cvo_batch_set_tail_scores),
 * slower for one pair alone on its cooperating workgroups. */
int cvo_set_tail_scores(cvo_handle h, int on);
int cvo_queued_score_count(cvo_handle h, int* count);   /* score blocks of this handle that were answered by what an alignment had queued */
/* pcd_generator::num_want (3000, pcd_generator.cpp:22) for this handle's later cvo_set_pcd_images calls */
int cvo_set_num_want(cvo_handle h, int num_want);
/* match_odometry / match_keyframe taking the images, exactly as the reference's signatures do */
int cvo_match_odometry_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height,
                              const cvo_camera* cam, double transform_out[12]);
int cvo_match_keyframe_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height,
                              const cvo_camera* cam, double transform_out[12]);
/* a slot's cloud back in the reference layout (xyz: n x 3, feat: 5 channel-major arrays of n); *n = points, cap = room in
 * the arrays (in points); nothing is written if cap < n */
int cvo_get_cloud(cvo_handle h, int slot, float* xyz, float* feat, int cap, int* n);
/* get_fixed_frame_selected_points / get_moving_frame_selected_points  cvo.hpp:272-276: pixel (x, y) of every point of a
 * cloud made by cvo_set_pcd_images (n x 2 uint16); *n = 0 for clouds handed in by cvo_set_pcd */
int cvo_get_selected_points(cvo_handle h, int slot, unsigned short* px, int cap, int* n);

/* ---- match_odometry / match_keyframe  cvo.cpp:461-473, 563-576:
 * set_pcd + align; transform_out = 3x4 row-major double (Affine3d). */
int cvo_match_odometry(cvo_handle h, const float* xyz, const float* feat, int n, double transform_out[12]);
int cvo_match_keyframe(cvo_handle h, const float* xyz, const float* feat, int n, double transform_out[12]);

/* ---- function_inner_product(cloud_a, cloud_b)  cvo.cpp:388-459 and
 * se3_Hessian(cloud_a, cloud_b, inliers)  cvo.cpp:620-759, on the handle's slots;
 * tran_a (may be NULL) is applied to slot a's positions first, as
 * compute_innerproduct does at cvo.cpp:485-487.  Both use the handle's CURRENT ell. */
int cvo_function_inner_product(cvo_handle h, int slot_a, const float* tran_a, int slot_b, cvo_inn_p* out);
int cvo_se3_hessian(cvo_handle h, int slot_a, const float* tran_a, int slot_b, double H[36], int* inliers /* in/out, accumulated */);

/* The same two members as the reference declares them -- function_inner_product(point_cloud* cloud_a, point_cloud* cloud_b)
 * cvo.hpp:222 and se3_Hessian(point_cloud* cloud_a, point_cloud* cloud_b, int& inliers) cvo.hpp:260 -- on clouds the caller
 * holds in host memory (reference layout: n x 3 positions, 5 channel-major feature arrays); the handle's CURRENT ell applies
 * (cvo.cpp:395, 626) and *inliers accumulates (cvo.cpp:708).  Both clouds are staged in scratch buffers of the handle. */
int cvo_function_inner_product_clouds(cvo_handle h, const float* xyz_a, const float* feat_a, int n_a,
                                      const float* xyz_b, const float* feat_b, int n_b, cvo_inn_p* out);
int cvo_se3_hessian_clouds(cvo_handle h, const float* xyz_a, const float* feat_a, int n_a,
                           const float* xyz_b, const float* feat_b, int n_b, double H[36], int* inliers /* in/out */);

/* ---- compute_innerproduct  cvo.cpp:475-503 */
int cvo_compute_innerproduct(cvo_handle h, cvo_inn_p* inn_pre, cvo_inn_p* inn_post, double post_hessian[36],
                             const float tran[12], int* inliers, cvo_inn_p* inn_fixed_pcd,
                             cvo_inn_p* inn_moving_pcd, float* cos_angle);
/* ---- compute_innerproduct_lc  cvo.cpp:505-561 */
int cvo_compute_innerproduct_lc(cvo_handle h, cvo_inn_p* inn_prior, cvo_inn_p* inn_lc_prior, cvo_inn_p* inn_lc_pre,
                                cvo_inn_p* inn_lc_post, double post_hessian[36], const float prior_tran[12],
                                const float lc_prior_tran[12], const float lc_prior_tran_2[12],
                                const float lc_tran[12], int* inliers_svd, int* inliers_pnpransac,
                                cvo_inn_p* inn_fixed_pcd, cvo_inn_p* inn_moving_pcd, float* cos_angle);

/* ---- cloud-slot state machine  cvo.cpp:578-618 */
int cvo_update_fixed_pcd(cvo_handle h);                                   /* cvo.cpp:578-582 */
int cvo_update_previous_pcd(cvo_handle h);                                /* cvo.cpp:584-589 */
int cvo_reset_keyframe(cvo_handle h, const float odometry[12]);           /* cvo.cpp:591-604 */
int cvo_reset_transform(cvo_handle h, const float odometry[12]);          /* cvo.cpp:606-609 */
int cvo_reset_initial(cvo_handle h, const float odometry[12], float init_inverse_out[12]);   /* cvo.cpp:611-618 */

/* ---- getters / public members  cvo.hpp:139-144, 268-270 */
int cvo_get_fixed_and_moving_number(cvo_handle h, int* fixed_num, int* moving_num);
int cvo_get_iteration_number(cvo_handle h, int* iteration);
int cvo_get_A_nonzero(cvo_handle h, int* nonzero);
int cvo_get_transform(cvo_handle h, float transform[12]);
int cvo_get_prev_accum_transform(cvo_handle h, float prev_transform[12], float accum_transform[12]);
int cvo_get_init(cvo_handle h, int* init);
int cvo_get_first_frame(cvo_handle h, int* first_frame);
int cvo_set_first_frame(cvo_handle h, int first_frame);
/* R, T (row-major 3x3, 3) and ell are private in the reference but are carried
 * state between calls (Q1, Q2); exposed so callers/tests can pin them. */
int cvo_get_state(cvo_handle h, float R[9], float T[3], float* ell);
int cvo_set_state(cvo_handle h, const float R[9], const float T[3], float ell);
/* number of workgroups that cooperate on this handle's alignment (latency knob; 0 = auto) */
int cvo_set_workgroups(cvo_handle h, int workgroups_per_pair);

/* ---- arithmetic modes: where a build of the reference with Eigen 3.3.7 rounds differently from this library's default (INTEGRATION.md,
 * "Eigen 3.3.7 arithmetic mode").  Each bit switches one part on its own; any subset is valid.  The bits equal the test oracle's
 * reference-noise variants (ORC_VAR_*), so one number selects the same reading on both sides.
 *   CVO_ARITH_F32_ROOTS   the step (cvo.cpp:76-92, 324-333) from the f32 eigenvalues of the companion matrix (f32 Hessenberg + Francis QR)
 *                         instead of the closed-form cubic
 *   CVO_ARITH_F32_LOGM    the second stop test's distance (cvo.cpp:94-104) as the Frobenius norm of an f32 matrix logarithm (Schur + Pade)
 *                         instead of the closed form
 *   CVO_ARITH_ROW_LAZY16  compute_flow's row sums `1/c*Ai*cross_xy`, `1/d*Ai*diff_yx` (cvo.cpp:222-223) with 1/c, 1/d folded into every
 *                         a_j before the sum in rows of fewer than 16 nonzeros (Eigen 3.3.7's lazy product), after it in longer rows
 * Default CVO_ARITH_BASE.  A handle's mode covers cvo_align(_traced), cvo_match_* (and their _images forms) and the score block in the
 * alignment's tail; a batch's covers cvo_batch_align_async and what is computed from its results (cvo_batch_compute_innerproduct_lc, the
 * gathered records).  The mode is taken when a launch is queued: launches already in flight keep theirs.  The adaptive-ell path
 * (cvo_adaptive_align) and the score kernels' own arithmetic have no modes.  Any other bit: CVO_ERR_INVALID. */
enum { CVO_ARITH_BASE = 0, CVO_ARITH_F32_ROOTS = 2, CVO_ARITH_F32_LOGM = 4, CVO_ARITH_ROW_LAZY16 = 8,
       CVO_ARITH_EIGEN337 = 2 | 4 | 8 };
int cvo_set_arith_mode(cvo_handle h, int flags);
int cvo_get_arith_mode(cvo_handle h, int* flags);

/* ---- adaptive-ell variant of the alignment: acvo::align, thirdparty/cvo/src/adaptive_cvo.cpp:490-555, with its
 * own constants (adaptive_cvo.cpp:27-46).  Per iteration the kernel matrices Axy, Axx and Ayy at the current ell give the length-scale
 * gradient dl (:154-272); ell moves by dl_step*dl inside [ell_min, ell_max], ell_max shrinking by 0.7 whenever it is hit (:538-545).
 * The reference's first loop never fills `sum_diff_yy_2` (:218-226 against :246-262): the rows of Ayy below num_fixed add nothing to
 * dl, only those from num_fixed on do; reproduced as is.  The reference does not build that file and has no caller for it
 * (thirdparty/cvo/CMakeLists.txt:66,77-81); its constants presume colour features scaled to [0,1] (c_ell = 0.5), which the shipped
 * generator does not produce (Q7).  A dense, untuned path: one workgroup per call.  Fresh-object semantics as after acvo::set_pcd
 * (ell = ell_init, ell_max as given, :476-477); R, T in: the start pose, out: the final one; transform_out = [R^T | -R^T T];
 * *iter = k at the break (left alone when max_iter is hit).  Clouds as for cvo_set_pcd.  trace may be NULL. */
typedef struct cvo_adaptive_params {
    float ell_init, ell_min, ell_max, dl_step;      /* 0.1, 0.0391, 0.15, 0.3        adaptive_cvo.cpp:27-32 */
    float sigma, sp_thres, c, d, c_ell, c_sigma;    /* 0.1, 8.315e-3, 7, 7, 0.5, 1   adaptive_cvo.cpp:35-42 (c_sp_thres = sp_thres) */
    int   max_iter; float min_step, eps, eps_2;     /* 2000, 0.2, 5e-5, 1e-5         adaptive_cvo.cpp:44-47 */
} cvo_adaptive_params;
typedef struct cvo_adaptive_row { float omega[3], v[3], dl, ell, step; int nnz_xy, nnz_xx, nnz_yy; } cvo_adaptive_row;
int cvo_adaptive_default_params(cvo_adaptive_params* p);
int cvo_adaptive_align(int device, const cvo_adaptive_params* p /* NULL = defaults */, const float* fixed_xyz, const float* fixed_feat, int n_fixed,
                       const float* moving_xyz, const float* moving_feat, int n_moving, float R_inout[9], float T_inout[3], float* ell_out,
                       float transform_out[12], int* iter, cvo_adaptive_row* trace, int trace_cap, int* trace_len);

/* ---- device self-test of the scalar closed forms the align kernel's epilogue runs once per iteration.  Each call
 * evaluates n cases on the device, one lane per case, with the very device functions the kernel calls:
 *   cubic_step: poly_solver + root selection + clamp, cvo.cpp:76-92,317-333   in: n x {c3, c2, c1, c0, min_step}  out: n steps
 *   exp_sek3:   Exp_SEK3 (K = 1) incl. the theta < 1e-6 branch, LieGroup.cpp:159-186   in: n x {omega[3], v[3], dt}
 *               out: n x {dR[9] row-major, dT[3]}
 *   dist_se3:   || logm([dR dT; 0 1]) ||_F, cvo.cpp:94-104   in: n x {dR[9], dT[3]}   out: n distances
 * Host pointers.  For known-answer tests that do not involve the CPU oracle (tests/test_gpu_closed_forms.py). */
int cvo_selftest_cubic_step(int device, int n, const float* coef_minstep, float* step_out);
int cvo_selftest_exp_sek3(int device, int n, const float* omega_v_dt, float* dR_dT_out);
int cvo_selftest_dist_se3(int device, int n, const float* dR_dT, float* dist_out);
/*   cubic_step_f32eig / dist_se3_f32logm: the same two in the arithmetic of CVO_ARITH_F32_ROOTS / CVO_ARITH_F32_LOGM (same layouts; a
 *               logarithm that fails gives NaN) */
int cvo_selftest_cubic_step_f32eig(int device, int n, const float* coef_minstep, float* step_out);
int cvo_selftest_dist_se3_f32logm(int device, int n, const float* dR_dT, float* dist_out);
/*   libm:       the device's float routines element by element: OCML's sinf, cosf, logf (logf: the gates, cvo.cpp:125-126) and the correctly rounded
 *               float sine and cosine Exp_SEK3 is evaluated with (LieGroup.cpp:174-175; cvo_math.hpp: sin_f32_cr, cos_f32_cr) and the correctly rounded logarithm of the
 *               gates (log_f32_cr)     in: n floats   out: n x {sinf, cosf, logf, sin_f32_cr, cos_f32_cr, log_f32_cr}
 *   pair_values: the pair arithmetic of se_kernel (cvo.cpp:166-175) by the four routes the align kernel has for it, for n pairs {fixed point at the
 *               origin with zero features; moving point y[3] with features g[5]} at length-scale `ell`:   in: n x {y0, y1, y2, g0, g1, g2, g3, g4}
 *               out: n x {a by the branchy full evaluation (dense fallback), a with the colour factor made once per list entry (lists outside the
 *               polynomial's range), a by the branch-free 12-term chain, a by the degree-7 polynomial with its rounding guard (the steady walk)} --
 *               a = 0 for a pair that is not a member of A; d2_d2c_out (may be NULL): n x {d2, d2c} as the device formed them.
 *               tests/test_gpu_pair_values.py: all four bit-equal to the oracle's (float)(s2*exp(-d2/(2.0*l*l))) sequence on >= 1e7 samples. */
/*   reset_initial: cvo::reset_initial (cvo.cpp:611-618) as the link kernel of the tracker streams evaluates it (cvo_tracks_step_async), with the very functions the
 *               host's cvo_reset_initial calls      in: n x {the object's transform[12], odometry[12]}   out: n x {R[9] row-major, T[3], init.inverse()[12]}
 *               tests/test_gpu_tracks.py: bit-equal to cvo_reset_initial on a handle and to the oracle */
int cvo_selftest_reset_initial(int device, int n, const float* transform_odometry, float* out);
int cvo_selftest_libm(int device, int n, const float* x, float* out6);
int cvo_selftest_pair_values(int device, const cvo_params* params /* NULL = defaults */, float ell, int n, const float* y_g, float* a_out, float* d2_d2c_out);
/*   voxel_slots: the two pure functions of the voxel-grid kernels' table ("Reducing clouds" and what follows it below), as those kernels call them, for n
 *               positions with features taken as zeros at voxel size `voxel` (finite, > 0) and a table of `slots` (>= 1) slots:   in: n x {x, y, z}
 *               out: valid_out[i] = 1 where the point is valid (belongs to a cell), key_out[i] = its cell's key (cx + 2^20) << 42 | (cy + 2^20) << 21 |
 *               (cz + 2^20), slot_out[i] = the slot at which the table starts to look for that key; 0 and 0 for an invalid point.
 *               tests/test_gpu_table_cases.py: equal to the numpy mirror (tests/table_cases.py), which places the engineered clouds' cells. */
int cvo_selftest_voxel_slots(int device, int n, const float* xyz, float voxel, unsigned slots, int* valid_out, unsigned long long* key_out, unsigned* slot_out);

/* ======================= batched alignment (independent frame pairs) ===========
 * keyframe<->keyframe loop-closure candidates (keyframe_graph.cpp:622-731) and
 * offline batches are independent cvo::cvo objects; a batch runs all of them in
 * one persistent launch, `workgroups_per_pair` workgroups each. */
typedef struct cvo_batch_s* cvo_batch;

typedef struct cvo_pair_result {       /* what match_keyframe + the getters return, per pair */
    float transform[12];               /* cvo::transform after align(), cvo.cpp:817 */
    float R[9];
    float T[3];
    float ell;                         /* ell left behind (Q1) */
    int   iter;                        /* get_iteration_number (Q4: value of k at the break; max_iter if none) */
    int   A_nonzero;                   /* get_A_nonzero (Q5) */
    int   iterations_run;              /* loop trips executed = iter+1 on a break */
    int   status;                      /* CVO_OK / CVO_ERR_* for this pair */
    int   rebuilds;                    /* dense O(N*M) culls executed (candidate lists are reused between them) */
    int   dense_fallbacks;             /* culls whose candidates overflowed the lists (slow per-row path taken) */
} cvo_pair_result;

int cvo_batch_create(const cvo_params* p, int device, int max_pairs, cvo_batch* out);
int cvo_batch_destroy(cvo_batch b);
/* upload pair p (host arrays, reference layout); sets R=I, T=0, ell=params.ell (fresh-object semantics) */
int cvo_batch_set_pair(cvo_batch b, int p, const float* fixed_xyz, const float* fixed_feat, int n_fixed,
                       const float* moving_xyz, const float* moving_feat, int n_moving);
/* the same for pairs first .. first+count-1 in one hand-over (arrays of `count` pointers / sizes): the clouds' arrays are copied as
 * they are into one pinned staging block, ONE host-to-device copy brings them over and ONE kernel builds the device layout -- the
 * way to hand a whole batch over per step (64 pairs of ~3 k points = 12.6 MB).  The host arrays may be reused when the call returns. */
/* Caller-registered host memory.  cvo_host_register pins a range of the caller's memory and maps it into the devices' address space (hipHostRegister); clouds that
 * cvo_batch_set_pair(s) is handed from INSIDE a registered range (both arrays of the cloud) are not copied at all: the align launch that builds their device layout
 * reads them over PCIe where they lie.  For them -- and only for them -- the arrays must stay valid and unchanged until that launch has been waited for (cvo_batch_wait);
 * everything else about the calls is unchanged, and clouds outside registered ranges are staged as before (cvo.cpp:345-386 copies its inputs too).  Register once, e.g.
 * the pool a frame grabber or dataset reader fills; cvo_host_unregister before the memory is freed. */
int cvo_host_register(void* ptr, size_t bytes);
int cvo_host_unregister(void* ptr);
int cvo_batch_set_pairs(cvo_batch b, int first, int count, const float* const* fixed_xyz, const float* const* fixed_feat, const int* n_fixed,
                        const float* const* moving_xyz, const float* const* moving_feat, const int* n_moving);
/* Pairs first .. first+count-1 from RGB-D images (the loop-closure batch of keyframe_graph.cpp:693-700 without a host round trip):
 * n_images distinct frames, all width x height, one camera, bgr8[i] (h x w x 3 bytes) and depth16[i] (h x w) each; every image is
 * generated ONCE on the GPU exactly as cvo_set_pcd_images would (pcd_generator + PixelSelector, the batch's num_want), all images by
 * one fixed list of launches with one host sync; pair k takes image fixed_image[k] as its fixed cloud and moving_image[k] as its moving
 * cloud (a reference frame shared by all candidates is listed once).  Fresh-object state like cvo_batch_set_pair (R = I, T = 0,
 * ell = params.ell); cvo_batch_set_state afterwards for reset_initial.  The images may be reused when the call returns.
 * points_out (n_images ints, may be NULL): the points of each generated cloud.  A bad index, a null pointer, a size below 64 or a
 * cloud above 65535 points fail with CVO_ERR_INVALID and no pair changes; an image that yields no points gives an empty cloud (the
 * align result of its pairs carries CVO_ERR_EMPTY_CLOUD).  Pairs outside the range keep their clouds. */
int cvo_batch_set_pairs_images(cvo_batch b, int first, int count, int n_images, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                               int width, int height, const cvo_camera* cam, const int* fixed_image, const int* moving_image, int* points_out);
/* pcd_generator::num_want (3000, pcd_generator.cpp:22) of this batch's later cvo_batch_set_pairs_images / cvo_batch_advance_images /
 * cvo_batch_stage_images calls; frames staged before (cvo_batch_stage_images) are dropped */
int cvo_batch_set_num_want(cvo_batch b, int num_want);

/* ---- K-stream frame-to-frame odometry: a pair slot as one cvo::cvo odometry object (the cvo_main loop: set_pcd, match_odometry,
 * update_fixed_pcd per frame, cvo.cpp:352-386, 461-473, 578-582), advanced by one frame per call, many slots per call.  Every result is
 * bit-identical to a handle given the same frames (cvo_set_pcd_images, cvo_match_odometry_images, cvo_update_fixed_pcd).
 *
 * cvo_batch_advance_images: image k (width x height, bgr8[k] and depth16[k] as for cvo_set_pcd_images) goes to slot slots[k], generated
 * once by the batched generator with camera cams[cam_index[k]] (cam_index NULL: cams[0] for every image) and the batch's num_want: cloud
 * and selected pixels are those cvo_set_pcd_images makes with that camera.  Per slot:
 *   - not started (a new slot, a plain pair, or after cvo_batch_reset_stream): the image becomes the FIXED cloud, nothing is aligned
 *     (cvo.cpp:352-360); a plain pair becomes a fresh stream first;
 *   - started: the moving cloud, if there is one, becomes the fixed cloud (update_fixed_pcd: a move of ownership, no copy and no new
 *     generation), the image becomes the MOVING cloud; R, T, ell, iter and the transforms carry on (cvo.cpp:461-473, 800-817).
 * A slot out of range or listed twice, a null pointer, a negative camera index, a size below 64 or a cloud above 65535 points fail with
 * CVO_ERR_INVALID and no slot changes.  An image with no points gives an empty cloud; the slot's alignments then carry the status a
 * handle's cvo_match_odometry_images returns (CVO_ERR_EMPTY_CLOUD).  points_out (count ints, may be NULL): the points of each cloud.
 *
 * cvo_batch_align_pairs_async: one persistent launch over the `count` listed slots, any subset in any order.  cvo_batch_wait results,
 * the tail scores / cvo_batch_innerproduct_results, the result records and the cvo_batch_last_* diagnostics are indexed in list order.
 * A listed stream slot without a moving cloud yet is not run: its entry carries CVO_ERR_NOT_INITIALIZED (cvo.cpp:463-466).  Slots not
 * listed keep their clouds and device states.  A stream slot starts from what it carries; a failed alignment leaves the slot as it was
 * (like a handle's).  Score blocks of the launch (cvo_batch_enqueue_innerproduct & co) fail with CVO_ERR_INVALID once one of its slots
 * has been advanced or reset.
 *
 * cvo_batch_reset_stream(b, p): slot p becomes a fresh object: no clouds, R = I, T = 0, ell = params.ell, every transform I -- the way to
 * reuse a slot for the next sequence.  cvo_batch_get_prev_accum_transform: cvo_get_prev_accum_transform of a stream slot (cvo.cpp:815-816).
 *
 * Interaction with the plain-pair calls: cvo_batch_set_pair, _set_pairs, _set_pairs_images and _set_state behave as before on any slot,
 * and on a stream slot they end the stream (the slot is a plain pair again).  cvo_batch_reset_states restores the plain pairs as before and
 * leaves the carried state of stream slots alone.  cvo_batch_align_async(b, n) is cvo_batch_align_pairs_async over slots 0 .. n-1, except
 * that every plain pair counts as started afterwards, as before. */
int cvo_batch_advance_images(cvo_batch b, int count, const int* slots, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                             int width, int height, const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */,
                             int* points_out /* may be NULL */);
int cvo_batch_reset_stream(cvo_batch b, int p);
int cvo_batch_align_pairs_async(cvo_batch b, int count, const int* slots, void* stream);
int cvo_batch_get_prev_accum_transform(cvo_batch b, int p, float prev_transform[12], float accum_transform[12]);

/* ---- The next frames of stream slots, staged ahead.  Frame t + 1's cloud depends on nothing that frame t's alignment produces, so it can be
 * generated while that alignment runs: stage the next frames right after cvo_batch_align_pairs_async, before cvo_batch_wait.
 *
 * cvo_batch_stage_images: the arguments of cvo_batch_advance_images.  The clouds of the `count` images are generated with the camera of
 * each and the batch's current num_want, on a stream of the stage's own (made with the device's highest stream priority, so that it does
 * not share a hardware queue with a running align launch) and in generator scratch of its own, into cloud objects that nothing else holds.
 * The call touches no slot, no stream state, no device state and no launch, and neither waits for nor disturbs a launch in flight.  It
 * returns without waiting for the device; every image byte has been copied to pinned memory by then (by the engine's copy threads), so the
 * caller may reuse the images at once.  It checks what cvo_batch_advance_images checks about its arguments (the list, null pointers, the
 * size limits, the camera index) and fails with CVO_ERR_INVALID before anything is staged: an earlier stage survives such a call.  There is
 * ONE stage per batch: a successful call replaces a stage that was never consumed, whose cloud objects return to the pool.
 * cvo_batch_set_num_want drops the stage, and so does a plain-pair call (cvo_batch_set_pair, _set_pairs, _set_pairs_images, _set_state) on
 * a staged slot.  cvo_batch_reset_stream keeps it: the staged frame is that slot's next frame, whatever the slot is by then.
 *
 * cvo_batch_advance_staged: cvo_batch_advance_images of the staged list, without generating anything -- it waits on the host only if the
 * staged generation has not finished (it needs the point counts), gives the staged cloud objects to the slots (the objects the slots let
 * go of are kept for later stages), and orders the launches that follow behind the stage's stream by an event.  The staged clouds arrive
 * with the boxes of their 32-point groups made, all of them by one launch.  Every result is bit-identical to cvo_batch_advance_images on
 * the same frames.  With nothing staged it returns CVO_ERR_INVALID.  A staged cloud above 65535 points (CVO_ERR_INVALID) or a HIP error of
 * the staged work (CVO_ERR_HIP) is reported here: no slot changes and the stage is dropped.  points_out: as for cvo_batch_advance_images.
 *
 * cvo_batch_staged_count: *images = images in the stage now (0 = none), *taken = clouds ever taken from a stage.  cvo_batch_destroy drains
 * the stage's stream first. */
int cvo_batch_stage_images(cvo_batch b, int count, const int* slots, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                           int width, int height, const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */);
int cvo_batch_advance_staged(cvo_batch b, int* points_out /* may be NULL, one int per staged image */);
int cvo_batch_staged_count(cvo_batch b, int* images /* may be NULL */, long long* taken /* may be NULL */);

/* ---- Frames that are already on the GPU (a decoder, a camera pipeline, a simulator, a torch tensor): the device twins of the image entry
 * points read caller-owned device memory, so nothing is copied to the host and back.  A call takes `count` descriptors, one per image, in
 * place of the two pointer arrays; everything else -- arguments, checks, results, the stage -- is its host twin's.  One kernel launch per
 * call (pcd_ingest_images_kernel) gathers all images into the generator's packed stacks; from there on the host twin's code runs, and every
 * result is bit-identical to the host twin given the same pixel values.
 *
 * Validation.  Every device entry point first runs the check that cvo_check_device_images runs alone, before any slot or stream changes
 * and before anything is queued: CVO_ERR_INVALID, the message naming image and field, for a null pointer, pixel_bytes not 3 or 4, swap_rb
 * not 0 or 1, a negative pitch or one below the row's bytes, depth16 or depth_pitch not 2-byte aligned, the size limits of the host twin,
 * and a pointer the device cannot read: hipPointerGetAttributes must report device memory of the object's device (and the image's rows,
 * [ptr, ptr + (height-1)*pitch + row bytes), must lie inside that allocation), managed memory, or pinned / registered host memory.  Pageable
 * host memory and memory of another device are refused and never reach a kernel.  The kernel reads nothing outside the rows: a row may end
 * where its allocation ends.
 *
 * Ordering.  The ingest ALWAYS runs on a stream of the library's own (the stage's high-priority stream for the stage calls, the object's
 * stream otherwise), never on the caller's: HIP deals streams of equal priority onto a few hardware queues, and a caller's stream that
 * shares the queue of a running align launch would not start before that launch ends.  image_stream says how the images' writer is ordered:
 *   image_stream != NULL: the library records an event on image_stream and its stream waits for it; behind the ingest it records a second
 *     event that image_stream waits for.  No host wait.  The images are the caller's again for any work queued on image_stream after the
 *     call has returned (work on other streams must be ordered behind image_stream by the caller).
 *   image_stream == NULL: the caller has already synchronised whatever wrote the images; the call waits on the host for the ingest alone
 *     (not for the generator) before it returns, and the images are the caller's again then.
 * The HIP null stream is handle 0, i.e. NULL: it cannot be named here and gets the host-waited form.  torch's default stream on ROCm is
 * that stream, so frames written on torch's default stream are passed with image_stream NULL after a synchronize of that stream; a
 * torch side stream (torch.cuda.Stream().cuda_stream) can be passed as image_stream. */
typedef struct cvo_device_image {
    const void* bgr8;        /* device-accessible; pixel (x, y) at bgr8 + y*bgr_pitch + x*pixel_bytes: bytes B, G, R (swap_rb: R, G, B); a 4th byte is ignored */
    const void* depth16;     /* device-accessible; uint16 at depth16 + y*depth_pitch + 2*x */
    long long bgr_pitch;     /* bytes per row; 0 = tight (width*pixel_bytes) */
    long long depth_pitch;   /* bytes per row; 0 = tight (2*width) */
    int pixel_bytes;         /* 3 or 4 */
    int swap_rb;             /* 0 / 1 */
} cvo_device_image;
int cvo_check_device_images(int device, int count, const cvo_device_image* images, int width, int height);   /* the validation alone: launches nothing */
int cvo_batch_set_pairs_device_images(cvo_batch b, int first, int count, int n_images, const cvo_device_image* images, int width, int height,
                                      const cvo_camera* cam, const int* fixed_image, const int* moving_image, int* points_out /* may be NULL */,
                                      void* image_stream);
int cvo_batch_advance_device_images(cvo_batch b, int count, const int* slots, const cvo_device_image* images, int width, int height,
                                    const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */, int* points_out /* may be NULL */,
                                    void* image_stream);
/* the ONE stage of the batch: replaces an unconsumed stage of either kind; cvo_batch_advance_staged consumes either kind, cvo_batch_staged_count counts both */
int cvo_batch_stage_device_images(cvo_batch b, int count, const int* slots, const cvo_device_image* images, int width, int height,
                                  const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */, void* image_stream);
/* The ingest kernel alone (tests): `count` images gathered into packed stacks that lie between 64 guard bytes on either side, prefilled with
 * 0xA5.  bgr_out: count*3*width*height bytes, depth_out: count*width*height uint16; *guards_intact = 1 when no guard byte changed. */
int cvo_selftest_ingest_images(int device, int count, const cvo_device_image* images, int width, int height, unsigned char* bgr_out,
                               unsigned short* depth_out, int* guards_intact);
/* ---- Clouds that are already on the GPU (the caller's own point selector, a learned feature extractor in torch, a lidar or stereo front end, a
 * simulator): the device twins of the cloud hand-over (cvo_batch_set_pair(s), and the K-stream steps, which have no host cloud form).  A call takes
 * `count` descriptors, one per cloud.  Validation, ordering and "a refused call changes nothing" are cvo_device_image's, rule for rule, with
 * cloud_stream in the place of image_stream; what differs is said here.
 *
 * Ingest is eager.  One kernel launch per call (cvo_ingest_clouds_kernel) copies all clouds of the call into cloud objects the library owns -- stream
 * slots and tracker objects hold a cloud for several steps -- and one more launch makes the boxes of their 32-point groups.  Both run on the object's
 * own stream, never on the caller's.  The caller's memory is the caller's again under image_stream's rule: with a cloud_stream an event edge in and an
 * event edge out; with NULL when the call has returned.  The host waits once per call, for the ingest launch alone, in either form: the launch leaves
 * each cloud's cost sample (cvo_batch_set_pairs' mean of 1/z^2 over every 16th point) in pinned memory, as the image path waits for its point
 * counts.  Every result is bit-identical to the same floats handed over from the host (cvo_batch_set_pairs; handles driven through cvo_set_pcd,
 * cvo_match_odometry, cvo_update_fixed_pcd).
 *
 * Validation: CVO_ERR_INVALID, the message naming cloud and field, for n outside 0 .. 65535; a stride that is negative or no multiple of 4;
 * xyz_stride in 1 .. 11; exactly one of the two feature strides 0; and, for n > 0, a null pointer, a base pointer that is not 4-byte aligned, and a
 * pointer the device cannot read, by the hipPointerGetAttributes rule of cvo_device_image with the extents
 *   [xyz, xyz + (n-1)*xyz_stride + 12)   and   [feat, feat + (n-1)*feat_point_stride + 4*feat_channel_stride + 4)
 * which must lie inside the allocation, and outside which the kernel reads nothing.  Pinned or registered host memory and managed memory are
 * accepted (a route for host callers); pageable host memory and another device's memory are refused.  n == 0 is valid and needs no pointers.
 *
 * cvo_batch_set_pairs_device_clouds: cvo_batch_set_pairs_images with clouds in place of generated images: n_clouds distinct clouds, pair k takes
 *   fixed_cloud[k] / moving_cloud[k]; a cloud listed for several pairs is ingested once and held by all of them; fresh-object state.
 * cvo_batch_advance_device_clouds: cvo_batch_advance_images per slot: a slot that has not started takes the cloud as its FIXED cloud, a started one
 *   does update_fixed_pcd by a move of ownership and takes the cloud as its MOVING cloud.  An unconsumed stage for a listed slot is dropped.
 * cvo_tracks_step_device_clouds_async (declared with the tracker steps below): cvo_tracks_step_async, the frame's cloud ingested once and held by
 *   both objects; cvo_track_step::points is n; n == 0 is an empty frame (CVO_ERR_EMPTY_CLOUD, the keyframe object left alone).
 * A slot or stream may receive images in one step and clouds in another.  For clouds handed over this way cvo_*_get_selected_points gives *n = 0
 * and cvo_*_get_cloud returns the floats that were handed over.  Reading the caller's device memory in place, without the copy, is not offered: it
 * would need cvo_host_register's lifetime contract. */
typedef struct cvo_device_cloud {
    const void* xyz;               /* float32, device-accessible; point i at xyz + i*xyz_stride: x, y, z */
    const void* feat;              /* float32; feature c (0..4) of point i at feat + i*feat_point_stride + c*feat_channel_stride */
    long long xyz_stride;          /* bytes; 0 = 12 (data_type.h:30) */
    long long feat_point_stride;   /* bytes; both feature strides 0 = the reference layout: 4 and 4*n (data_type.h:75) */
    long long feat_channel_stride;
    int n;                         /* 0 .. 65535 */
    int pad_;
} cvo_device_cloud;               /* 48 bytes */
int cvo_check_device_clouds(int device, int count, const cvo_device_cloud* clouds);      /* the validation alone: launches nothing */
int cvo_batch_set_pairs_device_clouds(cvo_batch b, int first, int count, int n_clouds, const cvo_device_cloud* clouds,
                                      const int* fixed_cloud, const int* moving_cloud, void* cloud_stream);
int cvo_batch_advance_device_clouds(cvo_batch b, int count, const int* slots, const cvo_device_cloud* clouds, void* cloud_stream);
/* The ingest kernel alone (tests): every cloud's planes lie between 64 guard bytes on either side, prefilled with 0xA5.  xyz_out: the clouds' n x 3
 * positions one cloud behind the other, feat_out: their 5 channel-major arrays of n likewise (the reference layout); cost_out: count x {sum of the
 * cost sample's terms, samples}; *guards_intact = 1 when no guard byte changed. */
int cvo_selftest_ingest_clouds(int device, int count, const cvo_device_cloud* clouds, float* xyz_out, float* feat_out,
                               double* cost_out /* count x {sum, samples} */, int* guards_intact);
/* ---- Reducing clouds (not in the reference): a voxel-grid filter in front of the device-cloud hand-over, which gives the cloud route the point
 * budget the image route has in num_want.  Many clouds per call; the result's bits depend on the input alone (no float atomics, no table order in
 * the output); the output is plain device memory that passes straight on as a cvo_device_cloud (xyz tight, feat "(n, 5)").
 *
 * The definition, for one cloud of n points (3 position and 5 feature floats), a voxel size (f32, finite, > 0), a mode and min_points >= 1:
 *   valid point: its 8 floats are finite and below 2^15 in magnitude, and each cell coordinate c = floorf(x / voxel) has |c| < 2^20 (the correctly
 *     rounded f32 division; floor, not truncation, for negative coordinates).  Invalid points belong to no cell.
 *   cell: the integer triple (cx, cy, cz); its members are the valid points with that triple; cells with fewer than min_points members are dropped.
 *   output order: ascending lowest member index of the cell; count[r] is row r's member count.
 *   CVO_REDUCE_MEAN: each of the row's 8 values is the members' mean in a form that does not depend on the order of summation: every member
 *     value v becomes q = llrint((double)v * 2^24), the q are added as 64-bit integers (2^20 points below 2^15: below 2^59), and the value is
 *     (float)((double)sum / ((double)count * 16777216.0)).  source[r] is the lowest member index.
 *   CVO_REDUCE_CENTRAL: the row is a copy of the 8 floats of the member nearest the cell's centre (c + 0.5f) * voxel (f32); d2 = dx*dx + dy*dy +
 *     dz*dz in f32, un-fused, added in that order; a tie goes to the lowest index.  source[r] is that member's index.
 *   map[i] (optional): the row of point i's cell, -1 for an invalid point or a dropped cell.
 *   The occupied-cell count of a cloud and a voxel size (cvo_count_voxels) is the number of cells with at least min_points members.
 *
 * A reducer owns its scratch -- sized at creation for max_clouds clouds of max_points points, 384 bytes per point (what 16 voxel sizes per cloud
 * need in cvo_count_voxels; a reduction uses under a third of it), never grown inside a call -- and its own stream.  All clouds of a call are
 * reduced by the same launches, the cloud in the grid's second dimension.  Input descriptors are cvo_device_clouds under cvo_check_device_clouds'
 * validation, rule for rule, except that n may go up to 1048575; further CVO_ERR_INVALID, the message naming cloud and field: n above max_points,
 * count above max_clouds, voxel not finite or not > 0, mode not 0 or 1, min_points < 1, cap outside 0 .. 65535, k outside 1 .. 16, and, in dst, a
 * null xyz or feat with cap > 0 or an array that is not 4-byte aligned device-writable memory of the reducer's device for its extent (xyz cap x 12,
 * feat cap x 20, count and source cap x 4, map n x 4 bytes; pageable host memory is refused).  A refused call changes nothing.
 * n_out[i] is always the FULL row count of cloud i; rows at or above cap are not written (no byte behind row cap - 1 is touched); map holds full
 * row numbers.  cap == 0 with every array NULL counts only.  cloud_stream: cvo_device_cloud's rule -- with a stream one event edge in and one
 * out, and the outputs are ordered on that stream; with NULL everything is done when the call returns.  The host waits once per call, for the
 * counts in pinned memory. */
#define CVO_REDUCE_MEAN 0
#define CVO_REDUCE_CENTRAL 1
#define CVO_REDUCE_MAX_POINTS 1048575
#define CVO_REDUCE_MAX_VOXELS 16
typedef struct cvo_reducer_s* cvo_reducer;
typedef struct cvo_reduce_params { float voxel; int mode; int min_points; int pad_; } cvo_reduce_params;   /* 16 bytes */
typedef struct cvo_reduced_cloud {      /* caller-owned DEVICE memory, one per input cloud */
    void* xyz;      /* cap x 3 float32, rows tight (12 bytes) */
    void* feat;     /* cap x 5 float32, rows tight (20 bytes): device_cloud's "(n, 5)" layout */
    void* count;    /* cap int32, may be NULL */
    void* source;   /* cap int32, may be NULL */
    void* map;      /* n_in int32, may be NULL */
    int cap; int pad_;
} cvo_reduced_cloud;                    /* 48 bytes */
int cvo_reducer_create(int device, int max_clouds /* 1 .. 4095 */, int max_points /* 1 .. 1048575 */, cvo_reducer* out);
int cvo_reducer_destroy(cvo_reducer r);
/* what the reducer was created with and the bytes of device scratch it holds (any pointer may be NULL) */
int cvo_reducer_info(cvo_reducer r, int* max_clouds, int* max_points, long long* scratch_bytes);
/* the validation of cvo_reduce_device_clouds alone: launches nothing */
int cvo_check_reduce_clouds(cvo_reducer r, int count, const cvo_device_cloud* in, const cvo_reduce_params* p, const cvo_reduced_cloud* dst);
int cvo_reduce_device_clouds(cvo_reducer r, int count, const cvo_device_cloud* in, const cvo_reduce_params* p /* one for all */,
                             const cvo_reduced_cloud* dst, int* n_out /* count, host */, void* cloud_stream);
/* the occupied-cell counts of all k voxel sizes of all clouds by one pair of launches over the count x k (cloud, size) items:
 * counts_out[i * k + j] for cloud i and voxels[j], equal to n_out of a reduction at that size */
int cvo_count_voxels(cvo_reducer r, int count, const cvo_device_cloud* in, int k, const float* voxels /* k */, int min_points,
                     int* counts_out /* count x k, host */, void* cloud_stream);
/* ---- Fusing clouds (not in the reference): a local map -- the clouds of the last K keyframes, each under its pose, merged into one voxel-reduced
 * cloud, with the cells that too few frames saw thrown away -- by the reducer's machinery: many groups per call, bits that depend on the input alone.
 *
 * The definition.  A fusion IS the reduction (above) of the concatenation of the moved members with the features unchanged, plus the views filter
 * and the two view outputs:
 *   group: a list of 1 .. 64 members; a member is a cvo_device_cloud (n up to 1048575, as for the reducer) and a pose: 12 f32, row-major 3 x 4 (the
 *     layout of cvo_point_support's tran), in HOST memory.
 *   global index: the group's points are the members' points, one member after the other: point i of member m has
 *     g = (sum of n of the members before m) + i.
 *   moved position: x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3] per row r, in f32 and un-fused (each product and sum rounded).  Features are
 *     not changed.
 *   valid point: its 8 source floats are finite and below 2^15 in magnitude, its 3 moved floats are finite and below 2^15, and each cell
 *     coordinate floorf(x' / voxel) has magnitude below 2^20.  From here on the reducer's definition applies to the sequence (moved position,
 *     features) in global-index order: cells, min_points, row order by ascending lowest global member index, MEAN by llrint(v * 2^24) integer
 *     sums, CENTRAL by the least (d2 bits, global index).  In CENTRAL the row's position is the winner's MOVED position, its features the copy.
 *   views: a cell's view mask is the 64-bit OR of 1 << m over its members' member numbers m (empty members keep their numbers); views is its
 *     popcount.  A cell is kept when it has at least min_points members AND at least min_views views (1 .. 64).  map is -1 for dropped cells.
 *   outputs per group, caller-owned device memory: xyz (cap x 3), feat (cap x 5); optional count, source (global index), views (int32), view_mask
 *     (uint64), each of cap rows; optional map, one int32 per global index.  n_out[g] is the FULL row count; rows at or above cap are not written
 *     and no byte behind row cap - 1 is touched.
 *
 * A fusion runs on an existing cvo_reducer and allocates nothing: a group takes the scratch region of one cloud (groups <= max_clouds, a group's
 * points <= max_points; its table has 2 x its points slots), the view masks lie in the part of the 384 bytes per point a reduction leaves unused
 * (cvo_reducer_info's scratch_bytes is what it was).  All groups and members of a call go through the same seven launches.  The poses travel with
 * the descriptor table in its one host-to-device copy.
 * Validation: CVO_ERR_INVALID, the message naming group, member and field, for everything cvo_check_reduce_clouds checks, per member cloud and per
 * dst array (view_mask needs 8-byte alignment, extent cap x 8; views cap x 4; map (group's points) x 4); group_first not ascending from 0; a group
 * with 0 or more than 64 members; more than 4096 members in the call; a group's points above max_points; groups outside 1 .. max_clouds; a pose
 * float that is not finite; min_views outside 1 .. 64.  A refused call changes nothing.  cloud_stream, the one host wait for the counts, and
 * cap == 0 with every array NULL meaning "count only" are cvo_reduce_device_clouds' rules. */
typedef struct cvo_fuse_member { cvo_device_cloud cloud; float pose[12]; } cvo_fuse_member;                 /* 96 bytes */
typedef struct cvo_fuse_params { float voxel; int mode; int min_points; int min_views; } cvo_fuse_params;    /* 16 bytes */
typedef struct cvo_fused_cloud {        /* caller-owned DEVICE memory, one per group; all but xyz and feat may be NULL */
    void* xyz;        /* cap x 3 float32 */
    void* feat;       /* cap x 5 float32 */
    void* count;      /* cap int32 */
    void* source;     /* cap int32: global index */
    void* map;        /* (group's points) int32 */
    void* views;      /* cap int32 */
    void* view_mask;  /* cap uint64 */
    int cap; int pad_;
} cvo_fused_cloud;                      /* 64 bytes */
/* the validation of cvo_fuse_device_clouds alone: launches nothing */
int cvo_check_fuse_clouds(cvo_reducer r, int groups, const int* group_first /* groups + 1 */, const cvo_fuse_member* members,
                          const cvo_fuse_params* p, const cvo_fused_cloud* dst);
int cvo_fuse_device_clouds(cvo_reducer r, int groups, const int* group_first /* groups + 1 */, const cvo_fuse_member* members,
                           const cvo_fuse_params* p /* one for all */, const cvo_fused_cloud* dst, int* n_out /* groups, host */, void* cloud_stream);
/* ---- Reducing frames (not in the reference): the reducer and the fuser reading RGB-D frames in place.  A lane takes a pixel and computes that
 * pixel's point on the fly, by the generator's own float sequence, so no dense cloud exists in memory and a reduced frame carries the numbers a
 * selected frame carries.  Everything behind the point -- table, rows, means, views -- is the machinery above.
 *
 * The dense cloud of a frame.  A frame is a cvo_device_image of width x height (w x h), a cvo_camera and a step in 1 .. 16.  With
 * ws = ceil(w / step) and hs = ceil(h / step) the cloud has n = ws * hs points; point i is pixel (x, y) = ((i % ws) * step, (i / ws) * step),
 * row-major over the sub-grid, and p = y * w + x is the pixel's flat index.
 *   position, all in f32, un-fused, in this order: z = (float)d / scaling_factor with d the uint16 depth; X = ((float)x - cx) * z / fx;
 *     Y = ((float)y - cy) * z / fy (pcd_generator.cpp:456-499).  d == 0 gives X = Y = Z = quiet NaN (0x7FC00000): the reducer's validity rule
 *     drops the point, no mask is needed.
 *   features 0 .. 2: the pixel's B, G, R bytes as floats; swap_rb is resolved as the ingest resolves it, so feature 0 is always B.
 *   features 3, 4: the generator's level-0 gradients on the FLAT index (pcd_generator.cpp:122-136): with
 *     I[q] = (float)((B*4899 + G*9617 + R*1868 + 8192) >> 14), for w <= p < w*(h-1): dx = 0.5f*(I[p+1] - I[p-1]), dy = 0.5f*(I[p+w] - I[p-w]);
 *     elsewhere both are 0.  Rows are not special: at x = 0 the left neighbour is the previous row's last pixel.  For a crop descriptor w, h and
 *     the neighbours are the crop's.  A step > 1 cloud is a row subset of the step-1 cloud: gradients always come from full-resolution neighbours.
 *   The kernels read no byte outside the image's rows.
 * The cloud that cvo_set_pcd_images generates from a frame is a row subset of the frame's step-1 dense cloud (the rows of its selected pixels
 * with d != 0), bit for bit.
 *
 * Reduction, counting and fusion of frames are exactly cvo_reduce_device_clouds, cvo_count_voxels and cvo_fuse_device_clouds applied to the
 * dense clouds: validity, cells, min_points, row order, MEAN and CENTRAL, cap, n_out, map, views, view_mask, global indices and "count only" are
 * those calls' rules, word for word.  map has n = ws * hs entries, one per sub-grid pixel.  In a fusion a member is {cvo_device_image, pose[12],
 * camera index}; all members of a call share width, height and step, their points are moved by the fuser's rule, and a group's points are
 * members * n <= max_points.  A frame's features are bounded by construction (bytes, and half differences of bytes), so a pixel's validity and
 * cell depend on its depth alone: the insert and count passes read 2 bytes per pixel; the gather recomputes position and features from the
 * pixel and its four flat neighbours; CENTRAL's write recomputes the winner.
 *
 * All calls work on an existing cvo_reducer and allocate nothing.  image_stream follows cvo_device_image's ordering rule with the reducer's
 * stream as the library's own: with a stream one event edge in and one out (the outputs are ordered on that stream), with NULL everything is
 * done when the call returns; the counts cost one host wait.
 * Validation (cvo_check_device_frames): cvo_check_device_images' rules on the reducer's device, and CVO_ERR_INVALID for step outside 1 .. 16,
 * count above max_clouds, ws * hs above max_points, a null cams, a cam_index entry that is negative (cam_index NULL: cams[0] for every frame;
 * cams holds max(cam_index) + 1 cameras), a camera float that is not finite, and scaling_factor, fx or fy equal to 0.  The reduce, count and fuse
 * calls add the checks of their cloud twins on params and dst (for a fusion: group_first, 1 .. 64 members per group, at most 4096 per call,
 * members * n <= max_points, finite poses, min_views).  A refused call changes nothing and launches nothing. */
typedef struct cvo_frame_cloud {        /* caller-owned DEVICE memory: one frame's dense cloud, n = ws * hs rows */
    void* xyz;      /* n x 3 float32, rows tight */
    void* feat;     /* n x 5 float32, rows tight: device_cloud's "(n, 5)" layout */
} cvo_frame_cloud;                      /* 16 bytes */
typedef struct cvo_fuse_frame { cvo_device_image image; float pose[12]; int cam; int pad_; } cvo_fuse_frame;   /* 96 bytes */
int cvo_check_device_frames(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                            const int* cam_index /* NULL: cams[0] for every frame */);
/* the dense clouds themselves, one launch for all frames: the definition made visible (dst arrays: 4-byte aligned device memory of n x 12 and
 * n x 20 bytes) */
int cvo_frames_to_device_clouds(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                                const int* cam_index, const cvo_frame_cloud* dst, void* image_stream);
int cvo_reduce_device_frames(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                             const int* cam_index, const cvo_reduce_params* p /* one for all */, const cvo_reduced_cloud* dst /* map: n entries */,
                             int* n_out /* count, host */, void* image_stream);
int cvo_count_frame_voxels(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                           const int* cam_index, int k, const float* voxels /* k */, int min_points, int* counts_out /* count x k, host */,
                           void* image_stream);
/* the validation of cvo_fuse_device_frames alone: launches nothing.  cams holds max(members[].cam) + 1 cameras */
int cvo_check_fuse_frames(cvo_reducer r, int groups, const int* group_first /* groups + 1 */, const cvo_fuse_frame* members, int width, int height,
                          int step, const cvo_camera* cams, const cvo_fuse_params* p, const cvo_fused_cloud* dst);
int cvo_fuse_device_frames(cvo_reducer r, int groups, const int* group_first /* groups + 1 */, const cvo_fuse_frame* members, int width, int height,
                           int step, const cvo_camera* cams, const cvo_fuse_params* p /* one for all */, const cvo_fused_cloud* dst,
                           int* n_out /* groups, host */, void* image_stream);
/* ---- Viewing clouds (not in the reference): a posed device cloud -- a fused local map -- seen from a camera: the z-buffered subset of its points
 * that the camera can see, which is what a frame-to-model tracker aligns against, and the z-buffer itself.  Many views per call; as in the
 * reducer the result's bits depend on the input alone (integer atomics only, no float atomics, no table or arrival order in any output).
 *
 * The definition.  A view is a cvo_device_cloud under the reducer's validation (n up to 1048575), a pose (12 f32, row-major 3 x 4, HOST memory)
 * taking the cloud's frame to the camera's frame, and a camera index into cams.  One cvo_view_params holds for all views of a call: width,
 * height, cell (1 .. 16), mode, z_near, z_far, slack, depth_tol; gw = ceil(width / cell), gh = ceil(height / cell).
 *   moved position: the fuser's rule, bit for bit: x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3] per row r, f32, un-fused.  Features pass
 *     through.
 *   valid point: the fuser's rule: its 8 source floats and its 3 moved floats are finite and below 2^15 in magnitude.
 *   in view: a valid point is in range when z_near <= z' && z' <= z_far.  Its image coordinates are u = (x' * fx) / z' + cx and
 *     v = (y' * fy) / z' + cy, in f32 with every product, quotient and sum rounded, in that order (the inverse of the generator's
 *     X = ((float)x - cx) * z / fx: every pixel of a frame with depth reprojects onto itself).  Both must be finite and below 2^20 in magnitude;
 *     px = (int)floorf(u + 0.5f), py = (int)floorf(v + 0.5f), and 0 <= px < width, 0 <= py < height.
 *   z-cell: (px / cell, py / cell); z-cell number (py / cell) * gw + px / cell.
 *   front: a z-cell's front is the in-view point with the least 64-bit key (bits of z' << 32) | index: z' > 0, so the bits order as the floats
 *     do; a tie in z' goes to the lowest index.
 *   visible: CVO_VIEW_FRONT: the fronts alone (at most gw * gh rows: cell is the point budget).  CVO_VIEW_SURFACE: every in-view point with
 *     z' <= zf + slack * zf, zf its z-cell's front depth, in f32 with product and sum rounded; slack = 0 keeps exactly the points whose z' equals
 *     the front's.
 *   rows: the visible points in ascending input index: a viewed cloud is a row subset of the moved cloud, in order.
 *   outputs per view, caller-owned device memory, all optional but xyz and feat: xyz (cap x 3, the moved position), feat (cap x 5, the "(n, 5)"
 *     layout: the result passes on as a cvo_device_cloud), source (cap int32, the input index), pixel (cap int32, py * width + px), relation
 *     (cap int32, below), map (n int32: the full row number if visible, -1 in view but hidden, -2 valid but out of range or outside the image,
 *     -3 invalid), depth (gw * gh f32: the front's z', 0 for an empty z-cell), index (gw * gh int32: the front's input index, -1 for an empty
 *     z-cell).  n_out[i] is always the FULL row count; cap is 0 .. 65535; rows at or above cap are not written and no byte behind row cap - 1
 *     is touched.  cap == 0 with the row arrays NULL counts only; depth, index and map may still be asked for.
 *   relation needs `observed`: one cvo_device_image per view, of width x height, of which only depth16 and depth_pitch are read and validated
 *     (NULL for the call: no relation is computed; a relation array without observed is refused).  For a row at (px, py) with observed d:
 *     d == 0 gives 0, unknown.  Otherwise zo = (float)d / scaling_factor and t = depth_tol * zo, in f32; z' < zo - t gives 1 (in front: the
 *     camera saw through the point), z' > zo + t gives 3 (behind), anything else 2 (agrees).  relation_counts (views x 4 ints, host, may be
 *     NULL) holds the four counts over ALL rows, those at or above cap included.
 *
 * A call runs on an existing cvo_reducer and allocates nothing.  A view takes one cloud's scratch region: its z-buffer (8 bytes x gw * gh), a
 * per-point z-cell or code word (4 bytes x n) and its per-block counts -- hence gw * gh <= max_points; cvo_reducer_info's scratch_bytes is what
 * it was.  The same cloud may appear in several views of one call (one map seen from K streams' predicted poses, or from K hypotheses).  All
 * views of a call go through the same launches, the view in the grid's second dimension; poses and cameras travel with the descriptor table.
 * Validation: CVO_ERR_INVALID, the message naming view and field, for everything cvo_check_reduce_clouds checks per cloud and per output array
 * (extents: pixel and relation cap x 4 bytes, depth and index gw * gh x 4, map n x 4); views outside 1 .. max_clouds; n > max_points;
 * gw * gh > max_points; width or height outside 1 .. 8192; cell outside 1 .. 16; mode not 0 or 1; z_near not finite or not > 0; z_far not
 * finite, not > z_near, or above 32768; slack or depth_tol not finite or negative; a pose float that is not finite; a negative camera index; a
 * camera float that is not finite, or fx, fy or scaling_factor equal to 0; observed with a null or misaligned depth16, a bad depth_pitch, or rows
 * outside a device-readable allocation (cvo_device_image's rule, for the depth plane only).  A refused call changes nothing and launches nothing.
 * cloud_stream: the reducer's rule -- with a stream one event edge in and one out, with NULL everything is done on return; one host wait, for
 * the counts. */
#define CVO_VIEW_FRONT 0
#define CVO_VIEW_SURFACE 1
typedef struct cvo_view { cvo_device_cloud cloud; float pose[12]; int cam; int pad_; } cvo_view;               /* 104 bytes */
typedef struct cvo_view_params { int width, height, cell, mode; float z_near, z_far, slack, depth_tol; } cvo_view_params;   /* 32 bytes */
typedef struct cvo_viewed_cloud { void *xyz, *feat, *source, *pixel, *relation, *map, *depth, *index; int cap; int pad_; } cvo_viewed_cloud;   /* 72 bytes */
/* the validation of cvo_view_device_clouds alone: launches nothing.  cams holds max(v[].cam) + 1 cameras */
int cvo_check_view_clouds(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p,
                          const cvo_device_image* observed /* NULL or views */, const cvo_viewed_cloud* dst);
int cvo_view_device_clouds(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p /* one for all */,
                           const cvo_device_image* observed /* NULL or views */, const cvo_viewed_cloud* dst, int* n_out /* views, host */,
                           int* relation_counts /* views x 4, host, may be NULL */, void* cloud_stream);
/* ---- Resident maps (not in the reference): voxel maps that stay in device memory between calls, one per tracker stream, to which posed clouds or
 * frames are added and from which they are taken away again.  A cvo_maps object holds max_maps independent maps of at most max_rows rows at one
 * voxel size.  It is created on an existing cvo_reducer: every call uses the reducer's scratch and stream, and nothing is allocated after
 * creation.  Every call takes a list of maps (each map at most once) and handles all of them in the same launches, the map in the grid's second
 * dimension.  As everywhere in the reducer, every output's bits depend on the calls alone: integer atomics only, and the table's layout never
 * shows.
 *
 * The definition, per map.
 *   row: a map is an ordered list of rows, one per cell that was ever occupied since the last compaction.  A row holds the cell key (the
 *     reducer's 63-bit key of the moved position at `voxel`), eight signed 64-bit sums of llrint((double)v * 2^24), count (unsigned), view_mask
 *     (64 bits), last_stamp and born (int32).  A table from key to row exists (2 x max_rows slots); nothing about it reaches an output.
 *   member: the fuser's member (cvo_fuse_member, or cvo_fuse_frame with width, height, step and cameras) plus an int32 stamp >= 0, one per member
 *     of the call, in HOST memory.  Moved position, validity and cell are the fuser's rules, bit for bit.
 *   the update's own cells: an update of one map with a group of 1 .. 64 members first forms the group's cells exactly as cvo_fuse_device_clouds /
 *     cvo_fuse_device_frames does in CVO_REDUCE_MEAN with min_points = min_views = 1 and the cap at the group's points: every cell with its
 *     undivided sums, its member count, its mask of member numbers and its rank in the fusion's row order (ascending lowest global index).
 *   integrate (sign = +1): every call-cell in rank order.  Key in the map: the sums are added, count += members, view_mask |= the OR of
 *     1 << (stamp & 63) over the members that touched the cell, last_stamp = max(last_stamp, those stamps), and if count was 0 (a dead row is
 *     revived) born = the least of those stamps.  Key absent: the cell is born; its row number is rows + (its rank among this call's born
 *     cells), sums, count and mask are the call's, born the least and last_stamp the largest of its stamps.
 *   remove (sign = -1), with the members, poses and stamps that were integrated: the sums and the count are subtracted, the stamps' bits are
 *     cleared, last_stamp and born stay.  A row whose count reaches 0 is dead: it keeps its place and its key until a compaction.
 *   remove what is still there (sign = -2, CVO_MAP_REMOVE_PRESENT): the removal for maps whose compactions drop LIVE rows (carving, probation;
 *     below).  Per call-cell, with B the OR of 1 << (stamp & 63) over the members that touched it: key absent -- the cell is skipped; the row's
 *     view_mask has none of B -- skipped (the row was dropped with these members in it and made again by others); it has all of B -- removed as
 *     by sign -1 (more members than the count: refused); it has some of B -- the call is refused.  This is exact as long as the stamps of the
 *     members a map holds are distinct modulo 64, and a group's members went in together or one per group (a group of one member can never
 *     be partly present).
 *   refusals after the count: an integration that would take rows above max_rows or a cell's count above 16777215 (under which the sums stay
 *     below 2^63), a removal of a cell that is absent or of more members than a cell's count: CVO_ERR_INVALID naming the first offending map
 *     of the call, with EVERY map unchanged.  For this an update runs in three steps: the fusion passes and a lookup-and-count pass; the call's
 *     one host wait, for the per-map figures; then the launches that write the maps, queued on the reducer's stream, behind which every later
 *     call on the reducer runs.  The members are read in the first step only.
 *   extract: map k is filtered by filter[k]: a row is kept when count >= max(1, min_points), popcount(view_mask) >= min_views and
 *     last_stamp >= min_last_stamp.  Kept rows go out in ascending row number.  xyz and feat are (float)((double)sum / ((double)count *
 *     16777216.0)), the reducer's MEAN expression: the result passes on as a cvo_device_cloud.  Optional outputs: count, views (int32),
 *     view_mask (uint64), last_stamp, born, row (int32: the map's row number).  cap (0 .. 65535), n_out (always the FULL count), "no byte behind
 *     row cap - 1" and "cap == 0 with every array NULL counts only" are cvo_reduce_device_clouds' rules.
 *   compact: map k takes keep[k] and optionally a device byte per row, drop[k].  A row stays when count >= 1, last_stamp >= min_last_stamp,
 *     (popcount(view_mask) >= min_views or born >= probation_from), and drop[k] is NULL or drop[k][row] == 0.  Surviving rows keep their order and
 *     are renumbered from 0; the table is rebuilt from them; new_row[k] (optional, device, one int32 per old row) gets each old row's new number
 *     or -1.  One call serves ageing, throwing out unconfirmed one-view cells after their probation, and free-space carving (drop from a view's
 *     relation == 1 through its source and extract's row).
 *   compaction and removal.  A compaction that drops only dead rows (min_last_stamp <= 0, min_views = 0, drop NULL) changes
 *     no later call.  One that drops LIVE rows -- drop, min_views with probation_from, min_last_stamp -- takes members' points out of the map for
 *     good: a later sign -1 removal of such a member is refused (its cell is absent), and if another member has made the cell again in between
 *     it is NOT refused and subtracts what the row never received: sign -1 after such a compaction is unsupported.  Remove those members with
 *     sign -2, which skips what is gone.  Then a map is no longer the fusion of its window: it is that fusion minus the dropped rows' members.
 *   extract's ceiling: cap is at most 65535 (what a hand-over takes) and there is no paging: a map may hold up to max_rows rows, but one
 *     extract call returns a map's kept rows whole only when the filter keeps at most 65535 (n_out still says how many there are).  For the
 *     part of a larger map that a camera sees, cvo_maps_view ("Viewing maps", below) reads the rows in place.
 *
 * Consequences (tests/map_reading.py restates the definition; the tests hold the kernels to it byte for byte).  Integrating one group in one
 * call with stamps 0 .. k-1 and extracting with (min_points, min_views) gives cvo_fuse_device_clouds' MEAN result for that group byte for byte
 * and in row order: xyz, feat, count, views, view_mask.  Integrating the same members in any split into consecutive calls gives the same bytes:
 * a cell is born in the earliest member that holds it and is ranked inside that call by lowest index -- ascending lowest global index -- and
 * integer sums do not care about grouping.  Removing a member gives, as a SET of rows, the fusion of the remaining members (sums, count and mean
 * bytes equal, mask bits at the stamps' positions) in the map's own order, birth order over its history: a sliding window costs two members a
 * step.  Extract, compact with a rule that drops nothing live, extract: the same bytes.
 *
 * Memory: per map and row 2 x 92 bytes (the rows exist twice: a compaction moves them from one side to the other, no lane waits for another)
 * and 24 for the table; cvo_maps_info gives the total.  In the reducer's scratch a group takes about 140 bytes per point of max_points;
 * cvo_maps_create refuses when max_maps groups do not fit.
 * Validation: CVO_ERR_INVALID, the message naming map, group, member and field: a null object; count / groups outside 1 .. max_maps; a map index
 * outside 0 .. max_maps - 1 or given twice; sign not +1, -1 or -2; a null or negative stamp; everything cvo_check_fuse_clouds / cvo_check_fuse_frames
 * checks on group_first, members, poses, cameras and the group's points against max_points; per extract output what cvo_check_fuse_clouds checks
 * on its arrays (view_mask 8-byte aligned; cap outside 0 .. 65535); min_views outside 0 .. 64; drop and new_row not device memory of `rows`
 * bytes / rows x 4 bytes.  At creation: max_maps outside 1 .. the reducer's max_clouds, max_rows outside 1 .. 1048575, voxel not finite or not
 * > 0.  A refused call changes nothing and launches nothing that writes a map.  stream: the fuser's cloud_stream / image_stream rule.
 * Destroy the maps before their reducer: cvo_reducer_destroy with live maps returns CVO_ERR_INVALID. */
#define CVO_MAP_MAX_ROWS 1048575
#define CVO_MAP_MAX_COUNT 16777215
#define CVO_MAP_INTEGRATE 1
#define CVO_MAP_REMOVE (-1)
#define CVO_MAP_REMOVE_PRESENT (-2)
typedef struct cvo_maps_s* cvo_maps;
typedef struct cvo_map_filter { int min_points; int min_views; int min_last_stamp; int pad_; } cvo_map_filter;         /* 16 bytes */
typedef struct cvo_map_keep { int min_last_stamp; int min_views; int probation_from; int pad_; } cvo_map_keep;         /* 16 bytes */
typedef struct cvo_map_cloud { void *xyz, *feat, *count, *views, *view_mask, *last_stamp, *born, *row; int cap; int pad_; } cvo_map_cloud;   /* 72 bytes */
int cvo_maps_create(cvo_reducer r, int max_maps, int max_rows, float voxel, cvo_maps* out);
int cvo_maps_destroy(cvo_maps m);
/* the creation values and the device bytes the object holds (any pointer may be NULL) */
int cvo_maps_info(cvo_maps m, int* max_maps, int* max_rows, float* voxel, long long* device_bytes);
/* the listed maps become empty */
int cvo_maps_clear(cvo_maps m, int count, const int* maps, void* stream);
/* rows[k]: map k's rows, dead ones included; live_rows[k]: those with count >= 1 (host arrays, either may be NULL; one host wait) */
int cvo_maps_rows(cvo_maps m, int count, const int* maps, int* rows, int* live_rows);
/* the validation of the update calls alone: launches nothing */
int cvo_check_maps_integrate_clouds(cvo_maps m, int groups, const int* maps /* groups */, const int* group_first /* groups + 1 */,
                                    const cvo_fuse_member* members, const int* stamps /* one per member */, int sign);
int cvo_check_maps_integrate_frames(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_frame* members, int width, int height,
                                    int step, const cvo_camera* cams, const int* stamps, int sign);
/* group g of the call goes into (sign +1) or out of (sign -1, or -2: what is still there) map maps[g] */
int cvo_maps_integrate_clouds(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_member* members, const int* stamps, int sign,
                              void* cloud_stream);
int cvo_maps_integrate_frames(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step,
                              const cvo_camera* cams, const int* stamps, int sign, void* image_stream);
int cvo_check_maps_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter /* count */, const cvo_map_cloud* dst /* count */);
int cvo_maps_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter, const cvo_map_cloud* dst, int* n_out /* count, host */, void* stream);
int cvo_check_maps_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep /* count */, const void* const* drop /* NULL, or count of NULL or device bytes */,
                           void* const* new_row /* NULL, or count of NULL or device int32 */);
int cvo_maps_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep, const void* const* drop, void* const* new_row,
                     int* rows_out /* count, host, may be NULL */, void* stream);
/* ---- Viewing maps (not in the reference): a resident map seen from a camera where it lies -- "Viewing clouds" with the map's rows as the
 * points, so that a tracker stream gets the part of its map a camera can see without cvo_maps_extract in between: no cloud of the whole
 * filtered map is written and read back, the filter may keep more than 65535 rows (the view's own output is what cap bounds), and free-space
 * carving is one byte array that cvo_maps_compact takes as it is.
 *
 * The definition.  A call is a list of VIEWS, not of maps: a cvo_map_view is a map number, a camera index into cams, a cvo_map_filter and a
 * pose (12 f32, row-major 3 x 4, HOST memory) taking the map's frame to the camera's frame.  The same map may stand in several views of one
 * call (one map under K hypotheses, or under K filters).  The call only reads the maps.  cvo_view_params and cvo_viewed_cloud are "Viewing
 * clouds"' as they stand.  Per view, with rows the map's row count, dead rows included:
 *   point index: the map's row number r in 0 .. rows - 1: the low word of the z-buffer key, the value in source and in the index image.
 *   filtered: row r takes part only if extract's rule keeps it under the view's filter: count >= max(1, min_points), popcount(view_mask) >=
 *     min_views, last_stamp >= min_last_stamp.  A row that is not kept has map[r] = -4 ("filtered or dead"); it is never divided, projected
 *     or counted.
 *   point: its eight floats are (float)((double)sum / ((double)count * 16777216.0)), extract's expression.
 *   valid point: the three mean position floats and the three moved floats are finite and below 2^15 in magnitude; otherwise map[r] = -3.
 *     The five feature means are NOT examined: in every supported map state a sum is the sum of llrint((double)v * 2^24) over `count` members
 *     with |v| < 2^15 (the fuser's validity).  The largest such f32 is 32768 - 2^-9, its llrint(v * 2^24) is exact, so |sum| <= count *
 *     (2^39 - 2^15) < 2^63.  The conversion of sum to f64, the division by the exact count * 2^24 and the conversion to f32 are each rounded
 *     to nearest and monotone; the first two move the bound 32768 - 2^-9 by a few units of 2^-38 at the most, and the last takes anything
 *     nearer than 2^-10 to that f32 back to it: the mean is below 2^15.  (A sign -1 removal after a
 *     compaction that dropped live rows is unsupported above and may break this.)  Project and count therefore read 24 of a row's 64 bytes of
 *     sums.  tests/map_view_reading.py asserts the condition on every kept row of every test.
 *   everything else is "Viewing clouds" word for word: the moved position, in view, z-cell, front (a tie in z' goes to the lowest row number),
 *     FRONT / SURFACE, rows in ascending index, pixel, relation, relation_counts, depth, index, n_out as the FULL count, cap in 0 .. 65535 with
 *     no byte touched behind row cap - 1, cap == 0 counting only.  dst.map has rows int32 entries.
 *   carve[k] (optional, needs observed): a device uint8 array of rows bytes.  Byte r is 1 when row r is visible in this view and its relation
 *     is 1 (the camera saw through it), 0 otherwise.  All rows bytes are written, computed over all visible rows, those at or above cap
 *     included.  It is cvo_maps_compact's drop as it is.
 * Consequence (tests/map_view_reading.py): with E the uncapped extract of the map under the view's filter and V the view of (E.xyz, E.feat),
 * n_out, xyz, feat, pixel, relation, relation_counts and depth are V's bytes; source = E.row[V.source]; index = E.row[V.index] where
 * V.index >= 0; map is -4 everywhere except map[E.row] = V.map; carve is 1 exactly at E.row[V.source[V.relation == 1]].  E.row is ascending,
 * so the front is the same: a view of a map is the view of its extract, without the extract and without its cap.
 *
 * Scratch: view q takes region q of the reducer's scratch, laid out from the call's own sizes, each array rounded up to 16 bytes: the z-buffer
 * 8 x gw * gh, a code word 4 x R, block counts 4 x B and block relation counts 16 x B, with R the most rows among the call's maps and
 * B = ceil(R / 256).  A region is an equal share of the scratch, cvo_reducer_info's scratch_bytes / max_clouds (384 bytes per point of
 * max_points), rounded down to 16.  A call whose layout is above it is refused, the message
 * naming both figures; a map may well have more rows than max_points.  Five of the reducer's counts per view.
 * Validation: CVO_ERR_INVALID, the message naming the view and the field: a null object or argument; views outside 1 .. the reducer's
 * max_clouds; a map index outside 0 .. max_maps - 1 (repeats are allowed); min_views outside 0 .. 64; everything cvo_check_view_clouds checks
 * on the parameters, poses, cameras, observed and, per output array, on dst (map: rows x 4 bytes); carve without observed; carve[k] that is
 * not device memory of rows bytes.  A refused call changes nothing and launches nothing; a successful call leaves every map byte-identical.
 * stream: the maps' rule -- the call is queued on the reducer's stream behind every earlier map write; with a stream one event edge in and
 * one out, with NULL everything is done on return; one host wait, for the counts.  observed, the output arrays and carve fall under that rule
 * as in cvo_view_device_clouds. */
typedef struct cvo_map_view { int map; int cam; cvo_map_filter filter; float pose[12]; } cvo_map_view;   /* 72 bytes */
/* the validation of cvo_maps_view alone: launches nothing.  cams holds max(v[].cam) + 1 cameras */
int cvo_check_maps_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p,
                        const cvo_device_image* observed /* NULL or views */, const cvo_viewed_cloud* dst, void* const* carve /* NULL, or views of NULL or device bytes */);
int cvo_maps_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p /* one for all */,
                  const cvo_device_image* observed, const cvo_viewed_cloud* dst, void* const* carve,
                  int* n_out /* views, host */, int* relation_counts /* views x 4, host, may be NULL */, void* stream);
/* ---- Probing maps (not in the reference): a resident map asked from the points' side -- for every point of a new cloud or frame under a pose,
 * the map row it falls into (reach 0) or lies nearest to among the 27 cells around it (reach 1).  One call answers what a frame-to-model front
 * end asks before it integrates a frame: how much of the frame is new to the map (the keyframe decision), which of its pixels land in a
 * confirmed cell (a static / known mask), and which row each point re-observes at what squared distance (association without an alignment).
 *
 * The definition.  A call is a list of PROBES, as a viewing call is a list of views: a cvo_map_probe is a map number, a cvo_map_filter and a
 * reach (0 or 1), and with it goes one posed member: a cvo_fuse_member (cvo_maps_probe_clouds), or a cvo_fuse_frame with the call's width,
 * height, step and cameras (cvo_maps_probe_frames); the pose takes the member's frame to the map's.  The same map may stand in several probes
 * of one call (one map under K pose hypotheses, one frame against K filters).  The call only reads the maps.  Per point i of the member (for a
 * frame: the fuser's sub-grid pixel index), with rows the map's row count, dead rows included:
 *   moved position, validity, cell: the fuser's rules, bit for bit: x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3] per row r, f32, un-fused;
 *     a point is valid when its source floats and its three moved floats are finite and below 2^15 in magnitude and each cell coordinate
 *     floorf(x' / voxel), at the maps' voxel, has magnitude below 2^20.  For a frame the source floats are the position alone, as in "Reducing
 *     frames".  An invalid point has row[i] = -3.
 *   reach 0: the point's own cell alone is examined.  Its key is absent from the map's table: row[i] = -1.  Present, but extract's rule under
 *     the probe's filter drops the row (count >= max(1, min_points), popcount(view_mask) >= min_views, last_stamp >= min_last_stamp; a dead
 *     row is always dropped): -4.  Otherwise row[i] is the row number.
 *   reach 1: the 27 cells c + d, d in {-1, 0, 1}^3, are examined.  A neighbour with a coordinate of magnitude 2^20 or more is in no map and is
 *     skipped; its key is never formed.  Among the examined cells whose row the filter keeps, the winner has the least (d2 bits, row number):
 *     CENTRAL's tie rule, a tie in d2 goes to the lowest row.  d2 = (dx*dx + dy*dy) + dz*dz in f32, every product and sum rounded, never
 *     contracted; dx = x' - mean_x with the mean extract's expression (float)((double)sum / ((double)count * 16777216.0)).  d2 >= 0, so its
 *     bits order as the floats do.  No cell kept: row[i] = -4 if at least one examined cell has a row in the table, -1 if none has.
 *   outputs per probe, caller-owned device memory, one entry per point, all optional: row (int32); dist2 (float32: the winner's d2, at reach 0
 *     the distance to the own cell's mean; bits 0x7F800000 where row < 0); count, views, last_stamp (int32: the winner row's count,
 *     popcount(view_mask) and last_stamp; 0 where row < 0); and hit (uint8), one byte per MAP row, `rows` bytes, dead rows included: byte r is 1
 *     when some point of this probe has row == r, else 0; all bytes are written.  dist2, count, views and last_stamp cannot stand without
 *     row; hit can.  With every array NULL the probe counts only.
 *   counts (host, 4 ints per probe, may be NULL): counts[4 * probe + k] is the number of points that are found (k = 0), absent (-1), filtered
 *     (-4) and invalid (-3); the four sum to the member's n.
 * The validity of a kept row's mean needs no test: the argument under "Viewing maps" applies unchanged (tests/map_probe_reading.py asserts it).
 *
 * A call runs on the maps' reducer and allocates nothing.  Probe q takes region q of the reducer's scratch -- an equal share,
 * cvo_reducer_info's scratch_bytes / max_clouds rounded down to 16 -- for its block counts, 16 bytes per 256 points; four of the reducer's
 * counts per probe.  Probes lie in 1 .. the reducer's max_clouds.  A member's n goes up to 1048575 and is not bound by max_points; a call
 * whose block counts are above a region is refused, the message naming both figures.  All probes go through the same two launches, the
 * probe in the grid's second dimension; no atomics: hit is cleared on the stream and set by byte stores of 1.
 * Validation: CVO_ERR_INVALID, the message naming the probe and the field: a null object or argument; probes outside 1 .. max_clouds; a map
 * index outside 0 .. max_maps - 1 (repeats are allowed); reach outside {0, 1}; min_views outside 0 .. 64; everything cvo_check_fuse_clouds /
 * cvo_check_fuse_frames checks on a member, its pose and its camera (n up to 1048575; a frame's ws * hs up to 1048575); per output array
 * 4-byte aligned device memory of n x 4 bytes, for hit of rows bytes; dist2, count, views or last_stamp without row.  A refused call
 * launches nothing; after any call every map is byte-identical.
 * stream: the maps' rule -- the call is queued on the reducer's stream behind every earlier map write; with a stream one event edge in and
 * one out, with NULL everything is done on return.  With counts the call has one host wait, for them.  With counts NULL and a stream it has
 * no host wait at all: the outputs are ordered on that stream.  (With counts NULL and a NULL stream the call waits for its own launches:
 * "done on return" is the only ordering such a caller has.) */
typedef struct cvo_map_probe { int map; int reach; cvo_map_filter filter; } cvo_map_probe;   /* 24 bytes */
typedef struct cvo_probed_points { void *row, *dist2, *count, *views, *last_stamp, *hit; } cvo_probed_points;   /* 48 bytes */
/* the validation of the probing calls alone: launches nothing.  cams holds max(members[].cam) + 1 cameras */
int cvo_check_maps_probe_clouds(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_member* members /* probes */,
                                const cvo_probed_points* dst /* probes */);
int cvo_check_maps_probe_frames(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_frame* members /* probes */, int width, int height,
                                int step, const cvo_camera* cams, const cvo_probed_points* dst);
int cvo_maps_probe_clouds(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_member* members, const cvo_probed_points* dst,
                          int* counts /* probes x 4, host, may be NULL */, void* cloud_stream);
int cvo_maps_probe_frames(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_frame* members, int width, int height, int step,
                          const cvo_camera* cams, const cvo_probed_points* dst, int* counts /* probes x 4, host, may be NULL */, void* image_stream);
/* ---- Saving and restoring maps (not in the reference): a resident map's rows copied out as they stand, and a map made of rows the caller
 * gives -- so that a map can grow (a new object with a larger max_rows, every map restored from the old one), outlast its process, move to
 * another reducer or another GPU, be forked into another slot to try something on a copy, and be put into a chosen state by a test.
 *
 * The statement.  The sums are integers and nothing about the table reaches an output, so a map IS its ordered rows: restoring the snapshot of
 * a map gives a map on which every later call -- integrate, remove, extract, compact, view, probe, snapshot -- returns the same bytes as on the
 * original (tests/map_snapshot_reading.py restates the definition; the tests hold the kernels to it byte for byte).
 *
 * A cvo_map_snapshot is six caller-owned DEVICE arrays, one set per map, a structure of arrays with row r at index r: keys (uint64), sums
 * (int64, 8 per row, row-major: a row's 64 bytes), count (uint32), view_mask (uint64), last_stamp and born (int32) -- 92 bytes a row -- and
 * rows: for a snapshot the arrays' capacity in rows, for a restore the rows to put in.
 *   snapshot: map maps[k]'s rows 0 .. rows - 1 are written to dst[k] as they stand, in row order, dead rows included (they keep their place
 *     and their key: a revival must find them).  dst[k].rows must be at least the map's rows, otherwise the call is refused with both
 *     figures: there are no partial snapshots.  No byte behind row rows - 1 of any array is touched.  rows_out[k] is the map's rows.  The
 *     call only reads the maps.  One launch for all listed maps.  The host knows every map's rows, so there is no host wait: with a stream
 *     one event edge in and one out (the maps' rule), with NULL everything is done on return.
 *   restore: map maps[k] becomes exactly the rows of src[k]: src[k].rows rows in order, the table built from their keys, the live count
 *     the rows with count >= 1.  What the map held before is gone.  voxel must have the bits of the object's voxel: a key means nothing at
 *     another cell size.  Source and destination may be different cvo_maps objects, on different reducers, with different max_rows.
 *   the rows are untrusted (they may come from a file): every row is tested on the device before any map changes, against the conditions of
 *     "every supported map state", so that a restored map is one that the arguments under "Viewing maps" and "Probing maps" cover.  The
 *     refusal bits, OR-ed over a map's rows:
 *        1  bad key: bit 63 set, or one of the three 21-bit fields 0.  A key is (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20) with
 *           |c| < 2^20, so every field lies in 1 .. 2^21 - 1.  (All ones is the table's empty mark.)
 *        2  count above CVO_MAP_MAX_COUNT.
 *        4  stamp: last_stamp < 0 or born < 0.
 *        8  sum out of bound: some |sum_k| > count * (2^39 - 2^15), as exact integers (the bound of "Viewing maps"; it implies eight zero
 *           sums in a dead row, and with a count that passes bit 2 the product is below 2^63).
 *       16  duplicate key: two rows of one map with the same key, among the rows whose key passes bit 1.
 *     A refusal is CVO_ERR_INVALID naming the first offending map in the call's order and its bits ("bits N"), and leaves EVERY listed map
 *     unchanged for every later call.  For this a restore runs in two steps, as an update does: the rows are written and tested on the side
 *     of the rows' memory that the map is not on, the table is emptied and the keys are inserted with the duplicate test; the call's one host
 *     wait, for the bits; then either the host flips the side and sets rows, or the launches that build every listed map's table again from
 *     the rows it still has (dead rows included, the live count counted again) are queued on the reducer's stream, behind which every later
 *     call on the reducer runs.  The caller's arrays are read in the first step only.
 * Validation: CVO_ERR_INVALID, launching nothing, the message naming map and field: everything the other map calls check on m, count and maps
 * (each map at most once); a null dst / src; an array that is null with rows to hold, is not device memory of the needed bytes (rows x 8, 64,
 * 4, 8, 4, 4; for a snapshot the MAP's rows) or is not aligned (keys, sums, view_mask 8 bytes, the others 4); a restore's rows outside 0 ..
 * max_rows of the destination (both figures in the message); voxel not the object's bits; a snapshot's capacity below the map's rows.
 * rows == 0 with NULL arrays restores an empty map and is legal. */
typedef struct cvo_map_snapshot { void *keys, *sums, *count, *view_mask, *last_stamp, *born; int rows; int pad_; } cvo_map_snapshot;   /* 56 bytes */
/* the validation of the two calls alone: launches nothing */
int cvo_check_maps_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst /* count */);
int cvo_maps_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst, int* rows_out /* count, host, may be NULL */, void* stream);
int cvo_check_maps_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src /* count */, float voxel);
int cvo_maps_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src, float voxel, void* stream);
/* ---- Merging maps (not in the reference): the first call that takes a MAP, not points -- the kept rows of a source map are added into a
 * destination map of the same voxel (level 0: the union of two streams' maps in one world frame, or of a fork and what it took in since) or of
 * a voxel 2^level times as large (level 1 .. 4: the whole map at a coarser voxel, under extract's 65535 rows and the align kernel's point
 * budget, without the keyframes it was made of).
 *
 * Why it is exact.  Cells nest: a cell coordinate is floorf(x / voxel) with a correctly rounded division; x / (voxel * 2^k) is x / voxel
 * divided by 2^k exactly (barring underflow), and floor(q / 2^k) == floor(floor(q) / 2^k): the cell of a point at voxel * 2^k is the arithmetic
 * right shift by k of its cell at voxel.  The sums are 64-bit integers: a coarse cell's sums, count and mask are the integer sum, sum and OR
 * of its children's.  A coarse map made from a fine map's rows is therefore, in key, sums, count, view_mask and last_stamp, row for row and in
 * order, dead rows included, the map that the same integrate and remove calls would have built at voxel * 2^k; born cannot be rebuilt from
 * rows (a coarse cell that never died keeps a stamp that its revived child has lost) and is defined below.
 *
 * The statement, per merge { dst_map, src_map, all_rows, filter } of a call with one `level` (tests/map_merge_reading.py restates it on
 * map_reading.Map; the kernels are held to it byte for byte): the kept rows of src_map are added into dst_map, each into the cell that its
 * own cell shifts to.
 *   which source rows are kept: with all_rows = 1 every row, dead rows included; otherwise those that extract's rule keeps under `filter`
 *     (count >= max(1, min_points), popcount(view_mask) >= min_views, last_stamp >= min_last_stamp): a dead row never passes it.
 *   where a row goes: its call-cell is its key with each of the three 21-bit cell fields c replaced by ((c - 2^20) >> level) + 2^20, an
 *     arithmetic shift.
 *   what a call-cell holds: sums and count, the integer sums over the kept rows it takes in; mask, the OR of their view_mask; hi, the largest
 *     last_stamp among them; lo, the least born among those with count >= 1, or if there are none the least born among all of them.
 *   order: call-cells are ordered by their lowest source row number.
 *   writing into the destination: a call-cell goes in as an integrate's call-cell does.  Absent in dst_map: a row is born behind the map's
 *     rows, in call-cell order, with the cell's key, sums, count and mask, last_stamp = hi and born = lo.  Present: the sums are added,
 *     count += count, view_mask |= mask, last_stamp = max(last_stamp, hi), and born = lo when the row was dead and the incoming count is at
 *     least 1.  The live count counts rows with count >= 1: a row that is born dead (a cell of dead rows alone) does not add to it.
 *   level 0 needs dst and src to have the same voxel bits; level k needs dst's voxel bits to be ldexpf(src's voxel, k).
 *   refusals after the count, as an update's: rows above dst's max_rows, or a resulting count above 16777215 (a call-cell's own count
 *     included: at level 4 a cell may take 4096 rows of 16777215; the sum is watched for the carry out of 32 bits and cannot wrap out of
 *     sight): CVO_ERR_INVALID naming the first offending merge and its destination map, with EVERY map unchanged.  A merge runs in an update's
 *     three steps: the call-cells formed from the sources' rows in the reducer's scratch and looked up in the destinations; the call's one
 *     host wait, for the figures; then the update's own launches that write the destinations, behind which every later call on the reducer
 *     runs.  The sources are read in the first step only.
 * dst and src are cvo_maps objects on one device; they may be the same object, and src may be on another reducer, with another max_rows.
 * A destination map stands at most once in a call; a source map may stand in several merges (one map into two destinations); within one
 * object a map that is both a source and a destination of the call is refused.  All merges go through the same launches, the merge in the
 * grid's second dimension.  The source is only read; the destination's table and rows are written by an update's born and update paths.
 * Integer atomics only (the key's compare-and-swap, the minimum of the lowest row, 32- and 64-bit integer adds, OR, max, min), no float atomics,
 * no lane waits for another; row order comes from ranks, never from arrival.
 *
 * Scratch: merge q forms its cells in region q of the DESTINATION's reducer's scratch, an update's region (about 140 bytes per point of
 * max_points): a source with more rows than that reducer's max_points is refused with both figures, as the views and probes refuse.
 * stream: the call runs on dst's reducer's stream under the maps' rule (one event edge in and one out with a stream, everything done on return
 * with NULL; one host wait, for the figures).  When src is on another reducer, ordering against src's writes is the caller's job: that is
 * restore's rule for its arrays.
 * Validation: CVO_ERR_INVALID, launching nothing, the message naming the merge and the field: a null object or argument; count outside 1 ..
 * dst's max_maps; level outside 0 .. 4; objects on different devices; voxel bits that do not match (both figures); dst_map / src_map outside
 * their object's maps; a destination listed twice; all_rows not 0 or 1; min_views outside 0 .. 64; a map that is source and destination; a
 * source with more rows than the destination's reducer's max_points.
 * Out of scope: merging under a pose (re-binning moved means is not exact); subtracting a merged map again; coarsening inside cvo_maps_view,
 * the probes or cvo_maps_extract (merge into a coarser object and view, probe or extract that). */
#define CVO_MAP_MERGE_MAX_LEVEL 4
typedef struct cvo_map_merge { int dst_map; int src_map; int all_rows; int pad_; cvo_map_filter filter; } cvo_map_merge;   /* 32 bytes */
/* the validation of cvo_maps_merge alone: launches nothing */
int cvo_check_maps_merge(cvo_maps dst, int count, const cvo_map_merge* merges /* count */, cvo_maps src, int level);
int cvo_maps_merge(cvo_maps dst, int count, const cvo_map_merge* merges, cvo_maps src, int level, void* stream);
/* pair p's cloud in slot CVO_SLOT_FIXED / CVO_SLOT_MOVING, as cvo_get_cloud / cvo_get_selected_points give a handle's
 * (selected pixels: clouds made by cvo_batch_set_pairs_images only, *n = 0 otherwise) */
int cvo_batch_get_cloud(cvo_batch b, int p, int slot, float* xyz, float* feat, int cap, int* n);
int cvo_batch_get_selected_points(cvo_batch b, int p, int slot, unsigned short* px, int cap, int* n);
/* warm start / carried ell for pair p (reset_initial + Q1) */
int cvo_batch_set_state(cvo_batch b, int p, const float R[9], const float T[3], float ell);
int cvo_batch_set_workgroups(cvo_batch b, int workgroups_per_pair /* 0 = auto: fill the CUs */);
/* cap on the workgroups one launch of this batch occupies (0 = no cap: up to the whole device).  Launches that are meant to run side
 * by side (several batches in flight on their own streams) each take a share; a launch with fewer pair slots than pairs hands its pairs
 * to the slots dynamically, so a slot is never idle behind the longest alignment. */
int cvo_batch_set_max_workgroups(cvo_batch b, int max_workgroups);
/* Adoption (off by default): in launches with one workgroup and one slot per pair, a workgroup that has finished its pair and finds
 * nothing queued on the device offers its help to a pair of the launch that still runs; from the next iteration on that pair runs on one
 * more workgroup (a pair can grow to four).  "Nothing queued" counts every align and score launch this library has submitted on the
 * device in this process, whatever its kind (not other processes, not other libraries' kernels).  Shortens the tail of a job whose
 * alignments take different numbers of iterations (33 ... 150); the results are those of any other workgroup count.
 * Helpers may also be launched with the pairs: when the launch's share of the device -- its workgroup slots divided by the align launches of
 * this library on the device that are estimated to run side by side, at most the hardware queues the runtime gives the process
 * (GPU_MAX_HW_QUEUES, read and never set; 4 when unset) -- holds more workgroups than it has pairs, the launch takes min(share,
 * 4 x pairs) workgroups and the extra ones join pairs from their first iterations.  A launch queued behind such launches on every hardware
 * queue does not count as "queued" for the helpers of the launches it waits for: it could not start before they end anyway.
 * A pair only counts on a helper that has CONFIRMED the acceptance of its offer; when no confirmation comes within 50 us the owner takes the
 * acceptance back and carries on with the workgroups it has -- a helper that disappears cannot turn a healthy pair into CVO_ERR_TIMEOUT.
 * cvo_batch_last_adoptions: pairs of the last launch that were helped; cvo_batch_last_adoption_retractions: acceptances taken back. */
int cvo_batch_set_adoption(cvo_batch b, int on);
/* arithmetic mode of the batch's launches queued after the call (CVO_ARITH_*, see cvo_set_arith_mode) */
int cvo_batch_set_arith_mode(cvo_batch b, int flags);
int cvo_batch_get_arith_mode(cvo_batch b, int* flags);
int cvo_batch_last_adoptions(cvo_batch b, int* pairs_helped);
int cvo_batch_last_adoption_retractions(cvo_batch b, int* retractions);
/* restore every pair's (R,T,ell) to what set_pair/set_state last gave it (bench loops re-run the same inputs) */
int cvo_batch_reset_states(cvo_batch b);
/* enqueue one persistent launch aligning pairs [0, n_pairs) on `stream` (a hipStream_t, NULL = the batch's own); asynchronous */
int cvo_batch_align_async(cvo_batch b, int n_pairs, void* stream);
/* wait for the launch and fetch results (n entries) */
int cvo_batch_wait(cvo_batch b, cvo_pair_result* results, int n);
/* has the last launch completed?  (never blocks; a caller that keeps several batches in flight can reuse whichever is done first --
 * alignments take data-dependent numbers of iterations, the oldest launch is not always the first to finish) */
int cvo_batch_done(cvo_batch b, int* done);
/* device time of the last launch in ms (HIP events on the launch stream), total loop trips it executed */
int cvo_batch_last_launch(cvo_batch b, float* kernel_ms, long long* iterations_total, long long* candidates_total);
/* the shape of the last launch: its workgroups, how many of them were launched as helpers (adoption), and the number of launches
 * (this one included) it was estimated to share the device with when it was submitted */
int cvo_batch_last_launch_shape(cvo_batch b, int* grid, int* helpers, int* concurrent);
/* The queue class of the batch's own stream, and how many hardware queues a class has (GPU_MAX_HW_QUEUES, read and never set; 4 when unset).
 * The HIP runtime keeps that limit per stream priority, so the library deals the streams of batch objects over two priorities: class 0 = normal
 * for the first `per_class_limit` objects alive on a device, class 1 = the least priority for the next as many, then whichever class has fewer.
 * Launches of class 1 yield to normal-priority work where both wait for a compute unit.  A class-1 object that plans a launch with more than one
 * workgroup per pair moves to class 0 first (cooperating workgroups never run below normal priority).  Handles, the batches inside a tracker
 * object and streams the caller passes are left alone.  CVO_HIP_QUEUE_CLASSES=0 (read once): every stream normal. */
int cvo_batch_queue_class(cvo_batch b, int* cls, int* per_class_limit);
/* nonzeros of the kernel matrix A (cvo.cpp:166-175) summed over every executed iteration of every pair of the last launch: the work the
 * reference's arithmetic is defined on (bench.py prices the kernel's instructions per nonzero with it) */
int cvo_batch_last_nonzeros(cvo_batch b, long long* nonzeros_total);
/* where the last launch spent its time: seconds summed over pairs, as seen by workgroup 0 of each pair:
 * [0] transform + list upkeep (cull, sort, refine)   [1] candidate phase   [2] candidates: workgroup reduction (incl. waiting
 * for the slowest wave)   [3] line-search phase   [4] candidates: exchange between the pair's workgroups   [5] scalar epilogue
 * [6] inside [0]: dense culls   [7] candidates: prologue   [8] inside [0]: row sorts   [9] candidates: the row walk */
int cvo_batch_last_phase_seconds(cvo_batch b, double seconds[10]);
/* seconds the first workgroup of each pair of the last launch spent on it (diagnostics: alignments take 33 ... 150 iterations of very different cost) */
int cvo_batch_last_pair_seconds(cvo_batch b, int n, double* seconds);
/* the same as spans on the device's own 100 MHz clock (one counter per device: the pairs of launches that ran side by side lie on one time axis), and the iteration
 * at which a finished workgroup joined the pair (0 = none; joined_at may be NULL): the drain of a job, pair by pair (scripts/gpu_timeline.py) */
int cvo_batch_last_pair_spans(cvo_batch b, int n, double* start_s, double* end_s, int* joined_at);
/* where the score block in the tail of the last launch spent its time (cvo_batch_set_tail_scores): seconds summed over pairs, workgroup 0 of each:
 * [0] final transform + list walk (inn_post, Hessian)   [1] the cull for inn_pre   [2] its walk + the rest   [3] all of it */
int cvo_batch_last_tail_seconds(cvo_batch b, double seconds[4]);
/* diagnostics: bit min(k, 63) of masks[i] is set when iteration k of pair i began with a dense cull (the candidate lists had gone stale, or were not there yet);
 * predicted[i] (may be NULL): the culls that built their lists around extrapolated positions */
int cvo_batch_last_cull_masks(cvo_batch b, int n, unsigned long long* masks, unsigned long long* predicted);
/* The last launch's results as records of CVO_RESULT_FLOATS floats {transform[12], iter, A_nonzero, iterations_run, status}: the
 * payload of the cross-GPU RCCL gather.  The align kernel writes them itself when a pair ends (no pack kernel behind the
 * launch): cvo_batch_result_records hands out the DEVICE address of the record table (valid once the launch's stream has drained; it
 * may move when a later launch has more pairs), cvo_batch_results_to_device copies the first n into a caller-owned DEVICE buffer
 * on `stream` (NULL = the launch's stream). */
#define CVO_RESULT_FLOATS 16
int cvo_batch_results_to_device(cvo_batch b, void* dst_device, int n, void* stream);
int cvo_batch_result_records(cvo_batch b, const void** records_device);

/* ======================= multi-GPU: shard the pairs, gather the SE(3) records ===========
 * Frame pairs are independent (loop-closure candidates keyframe_graph.cpp:622-731, offline batches): pair p of P goes to
 * a contiguous block per rank (cvo_shard_range: block sizes differ by at most one -- the reference's batch source is <= 10 loop-closure
 * candidates, i.e. 2,2,1,1,1,1,1,1 over 8 GPUs), its clouds live only on the owning GPU, and the ONLY exchange is one RCCL
 * all-gather of the CVO_RESULT_FLOATS-float result records over xGMI.  RCCL (librccl.so.1) is loaded when the first
 * communicator is made; a process that never shards does not need it.
 *
 * One process per GPU (torch.distributed / MPI launchers): rank 0 calls cvo_comm_unique_id, the host framework
 * broadcasts the CVO_COMM_ID_BYTES bytes, every rank calls cvo_comm_create (ncclCommInitRank).  One process, several
 * GPUs: cvo_comm_create_all (ncclCommInitAll).
 *
 * The gather.  An all-gather needs the same count on every rank, so every rank contributes a block of n_block =
 * cvo_shard_block(P, n_ranks) records: its n_valid own ones (written by the align kernel) and, behind them, records that stand for
 * no pair (status CVO_ERR_PADDING, the rest zero).  cvo_batch_gather_results_padded enqueues ONE ncclAllGather of n_block *
 * CVO_RESULT_FLOATS floats behind the launch on its stream: no host synchronisation between align and gather; recv_device
 * (n_ranks * n_block records, rank-major) is valid when that stream has drained (cvo_batch_wait); cvo_compact_records turns the
 * gathered table (on the host) into the P records in global pair order and reports the first non-zero status.
 * RULE: every rank enters the collective exactly once per step, whatever happened before.  A rank whose cvo_batch_align_async
 * failed passes that code as launch_status (n_valid is then ignored): all its records carry the status, its peers see it in the
 * gathered table instead of waiting for the rank forever.  A rank with no pairs (n_valid = 0) just sends padding.  Everything
 * that can fail inside the call (argument checks, buffer growth, the padding kernel) happens before the collective is posted, and a
 * rank on which it does fail STILL posts the all-gather -- from a block of CVO_ERR_RANK_FAILED records the communicator has held since
 * cvo_comm_create (1024 records; grown on demand) -- and then returns the error: its peers find status 8 in the gathered table
 * (cvo_compact_records' first_error).  Only when even that block is unavailable does the call return without entering the collective;
 * cvo_last_error() then ends in "(collective NOT entered)" and the peers have to be told out of band.
 * cvo_batch_gather_results(b, c, n, recv) is the n_valid = n_block = n form: n MUST be the same on every rank. */
#define CVO_COMM_ID_BYTES 128
typedef struct cvo_comm_s* cvo_comm;
int cvo_shard_range(int n_pairs_total, int rank, int n_ranks, int* first, int* count);    /* contiguous block of rank */
int cvo_shard_block(int n_pairs_total, int n_ranks);                                      /* records per rank in a gather: ceil(P / n_ranks) */
int cvo_comm_unique_id(char id[CVO_COMM_ID_BYTES]);
int cvo_comm_create(const char id[CVO_COMM_ID_BYTES], int n_ranks, int rank, int device, cvo_comm* out);
int cvo_comm_create_all(const int* devices, int n_devices, cvo_comm* out /* n_devices handles */);
int cvo_comm_info(cvo_comm c, int* n_ranks, int* rank);                                    /* ncclCommCount / ncclCommUserRank of the communicator */
int cvo_comm_destroy(cvo_comm c);
/* ORDER INVARIANT of the gathers: a communicator carries ONE gather per step, and every rank posts its gathers in the same (step) order.  Several may be
 * outstanding at once, on different streams (each behind the align launch it belongs to: bench.py keeps eight steps in flight), and a rank may post step k's
 * gather from whichever of its batch objects holds step k -- what has to agree across the ranks is the ORDER of the calls on the communicator, not the batch
 * object or the stream.  A rank that skips a step, or posts two steps in the other order, pairs its collective with the wrong one of its peers'.
 * cvo_comm_set_gather_stream(c, 1) (or CVO_HIP_GATHER_STREAM=1 when the communicator is made) posts every gather of the communicator to ONE stream of the
 * communicator's own instead -- behind an event of the align launch, with the launch's stream continuing behind the gather -- for a RCCL build that does not
 * take collectives of one communicator from several streams at once; cvo_batch_wait still returns with every rank's records in place.
 * cvo_comm_library_path: the file the bound RCCL was loaded from (a torch process resolves librccl.so.1 to torch's bundled copy, a C++ caller to /opt/rocm's). */
int cvo_comm_set_gather_stream(cvo_comm c, int on);
int cvo_comm_library_path(char* out, int cap);
int cvo_batch_gather_results(cvo_batch b, cvo_comm c, int n, void* recv_device);
int cvo_batch_gather_results_padded(cvo_batch b, cvo_comm c, int n_valid, int n_block, int launch_status, void* recv_device);
/* the block a rank would send (padding / status records in place), for launchers that run their own collective: DEVICE address,
 * complete in the order of the launch's stream */
int cvo_batch_padded_records(cvo_batch b, int n_valid, int n_block, int launch_status, const void** send_device);
int cvo_compact_records(const float* gathered_host, int n_pairs_total, int n_ranks, float* out_host /* n_pairs_total records */, int* first_error);
/* single-process form: one batch per device, all n_devices all-gathers inside one RCCL group (everything that can fail is checked
 * for every device before the group is opened) */
int cvo_gather_results(cvo_batch* batches, cvo_comm* comms, int n_devices, int n, void* const* recv_device);
int cvo_gather_results_padded(cvo_batch* batches, cvo_comm* comms, int n_devices, const int* n_valid, int n_block, const int* launch_status /* NULL = all CVO_OK */,
                              void* const* recv_device);

/* Convenience object for the single-process case: n_devices batches (one per GPU, max_pairs_per_device each), their
 * communicators and gather buffers.  cvo_multi_batch hands out device i's batch for cvo_batch_set_pair & co;
 * cvo_multi_align_async launches every device's batch (n pairs each) and enqueues the gather behind it;
 * cvo_multi_wait drains the streams and copies the gathered records (n_devices*n, device-major) to the host from
 * device `from_device`'s copy (every device holds all of them). */
typedef struct cvo_multi_s* cvo_multi;
int cvo_multi_create(const cvo_params* p, const int* devices, int n_devices, int max_pairs_per_device, cvo_multi* out);
int cvo_multi_destroy(cvo_multi m);
int cvo_multi_batch(cvo_multi m, int i, cvo_batch* out);
int cvo_multi_align_async(cvo_multi m, int n);
/* n_pairs[i] pairs on device i (0 = none); every device contributes max(n_pairs) records to the gather, padding behind its own */
int cvo_multi_align_async_v(cvo_multi m, const int* n_pairs);
int cvo_multi_wait(cvo_multi m, int from_device, float* records_out /* n_devices * max(n_pairs) * CVO_RESULT_FLOATS */);

/* Loop-closure verification of the aligned pairs (keyframe_graph.cpp:704-717): per pair the
 * compute_innerproduct_lc block (cvo.cpp:505-561: 6 inner products + 2 Hessians, lc_tran = the pair's
 * own align() result, ell = what that align() left behind, Q1) and the reference's accept rule.  All
 * pairs' 8 evaluations are ONE launch.  prior_tran / lc_prior_tran / lc_prior_tran_2: n row-major 3x4
 * Affine3f each (keyframe_graph.cpp: prior, lc_prior, lc_prior_2).  Waits for the align launch first. */
typedef struct cvo_lc_scores {
    cvo_inn_p inn_prior, inn_lc_prior, inn_pre, inn_post, inn_fixed_pcd, inn_moving_pcd;   /* cvo.cpp:539-551 */
    double post_hessian[36];           /* cvo.cpp:555 */
    int    inliers_svd;                /* cvo.cpp:554-555 */
    int    inliers_pnpransac;          /* cvo.cpp:557-558 */
    float  cos_angle;                  /* cvo.cpp:552 */
    int    accept;                     /* keyframe_graph.cpp:711-712: inn_post > inn_pre, inn_lc_prior, inn_prior and cos_angle >= 0.1 */
} cvo_lc_scores;
int cvo_batch_compute_innerproduct_lc(cvo_batch b, int n, const float* prior_tran, const float* lc_prior_tran,
                                      const float* lc_prior_tran_2, cvo_lc_scores* out);

/* The tracker's score block (cvo::compute_innerproduct, cvo.cpp:475-503; caller local_tracker.cpp:240-251) for the
 * first n pairs of the last align launch: tran = each pair's own align() result, ell = what that align() left
 * behind (Q1), inliers counted from 0.  enqueue queues ONE launch behind the align launch on its stream (the
 * transforms are read from the device-resident states, the host does not wait); results waits for it and finishes
 * the sums (inn_p count rule, Hessian scaling and eigenvalue shift) on the host.  compute = both. */
typedef struct cvo_track_scores {
    cvo_inn_p inn_pre, inn_post, inn_fixed_pcd, inn_moving_pcd;    /* cvo.cpp:489-497 */
    double post_hessian[36];           /* cvo.cpp:500 */
    int    inliers;                    /* cvo.cpp:708 */
    float  cos_angle;                  /* cvo.cpp:498 */
} cvo_track_scores;
int cvo_batch_enqueue_innerproduct(cvo_batch b, int n);
/* The same block answered by the align launch itself (off by default): when a pair's workgroup has finished the alignment it computes
 * inn_post and the Hessian terms from its resident candidate lists (the cloud re-transformed with the FINAL transform, cvo.cpp:485-487),
 * inn_pre from one cull of the untransformed cloud, and takes fip(fixed, fixed) / fip(moving, moving) from the clouds' tables of cached
 * self inner products -- no score launch has to find room beside the persistent align workgroups.  cvo_batch_innerproduct_results then
 * returns these; anything a workgroup could not answer (lists stale for the final transform, a pair run by several workgroups, a cloud
 * whose self product has not been computed yet) is computed by the score kernel at that point. */
int cvo_batch_set_tail_scores(cvo_batch b, int on);
/* which requests the last launch's workgroups answered themselves, per pair: bit 0 inn_pre, 1 inn_post, 2 inn_fixed_pcd, 3 inn_moving_pcd,
 * 4 the Hessian (diagnostics / tests; call before cvo_batch_innerproduct_results) */
int cvo_batch_last_tail_answers(cvo_batch b, int n, int* masks);
int cvo_batch_innerproduct_results(cvo_batch b, int n, cvo_track_scores* out);
int cvo_batch_compute_innerproduct(cvo_batch b, int n, cvo_track_scores* out);


/* ======================= K-stream tracker steps: the tracker's TWO objects per stream ===========
 * local_tracker runs two cvo::cvo objects per frame (local_tracker.cpp:228-251, 330-338, 356-431, 506): cvo_odometry aligns the frame to the previous
 * frame, cvo_keyframe aligns the same frame to the current keyframe, warm-started from the odometry result by reset_initial (cvo.cpp:611-618) and moved
 * on, after the caller's accept decision, by update_previous_pcd or reset_keyframe (cvo.cpp:584-604).  A cvo_tracks object is K such pairs of objects.
 * The accept rule stays with the caller; everything cvo::cvo does around it is done here, and every result is bit-identical to two handles driven
 * through cvo_set_pcd_images, cvo_match_odometry_images, cvo_update_fixed_pcd, cvo_reset_initial, cvo_match_keyframe_images, cvo_update_previous_pcd /
 * cvo_reset_keyframe (cvo_slam_amd/replay.py: replay_tracker is that loop).
 *
 * cvo_tracks_step_async: image k (as for cvo_batch_advance_images: one size per call, camera cams[cam_index[k]]) is the next frame of stream streams[k].
 * The frame is generated ONCE; its cloud is the moving cloud of both objects and becomes the odometry object's fixed cloud at the stream's next step.
 * By the frames a stream has seen:
 *   phase 0 (first frame)   it becomes the FIXED cloud of both objects (local_tracker.cpp:228, 231); nothing is aligned.
 *   phase 1 (second frame)  odometry: match_odometry and its score block (:233, :251).  When the step is waited for, the keyframe object gets
 *                           first_frame = false; reset_transform(t_odometry) (:330-333); it does not see this frame.  No decision is expected.
 *   phase 2 (later frames)  odometry alignment and score block (:356, :375); then on the keyframe object reset_initial(t_odometry) (:407),
 *                           match_keyframe of the same frame (:415) and its score block (:431).  The stream's next step fails with CVO_ERR_INVALID
 *                           until cvo_tracks_commit has been given the decision: accept != 0 update_previous_pcd (:506), accept == 0
 *                           reset_keyframe(t_odometry) (:337 via :518; both branches of cvo.cpp:593-601).
 * All of a step is queued without a host wait in between (the generator's one sync aside): ONE odometry launch over the listed streams, a link kernel
 * that evaluates reset_initial on the device from the odometry launch's device-resident results, ONE keyframe launch over the phase-2 streams that
 * starts from the states the link kernel wrote; both launches answer their score blocks in their tails (what a tail leaves open goes to the score
 * kernel at cvo_tracks_wait).  hip_stream: a hipStream_t for the launches (NULL = the object's own).  One step is in flight at a time.
 *
 * A stream whose odometry alignment did not return CVO_OK (an empty frame: CVO_ERR_EMPTY_CLOUD, as a handle gives) leaves its keyframe object exactly
 * as it was: keyframe.status is CVO_ERR_NOT_INITIALIZED, no decision is expected, a keyframe result computed anyway is dropped.  Its odometry object
 * still moves on at the next step (update_fixed_pcd), as the two-handle loop does.  A keyframe alignment that itself fails is reported in
 * keyframe.status; R and T stay as reset_initial set them, everything else is as it was, and a decision is expected as usual.  Argument errors -- a
 * stream out of range or listed twice, a null pointer, the size limits of cvo_batch_advance_images, a step for a stream whose decision is pending, a
 * decision for a stream that expects none -- fail with CVO_ERR_INVALID before any stream changes.
 *
 * cvo_tracks_wait: the results of the step in flight, one cvo_track_step per listed stream in list order (count = the step's count).  Entries of an
 * object that did not align carry status CVO_ERR_NOT_INITIALIZED and zeros.  cvo_tracks_done never blocks.
 * cvo_tracks_reset(t, s): stream s = two fresh objects.  cvo_tracks_get_cloud / _get_selected_points / _get_state: object 0 = odometry, 1 = keyframe;
 * slot CVO_SLOT_FIXED / _MOVING / _PREVIOUS (the odometry object has no previous cloud: *n = 0).
 *
 * The next step's frames, staged ahead (the stage of cvo_batch_stage_images, for streams): call cvo_tracks_stage_async for step f + 1 between
 * cvo_tracks_step_async / cvo_tracks_step_staged_async of step f and its cvo_tracks_wait -- staging while a step is in flight is the intended use.
 * cvo_tracks_stage_async takes cvo_tracks_step_async's arguments but the stream handle, checks what that call checks about them (the list, null
 * pointers, the size limits, the camera index: CVO_ERR_INVALID before anything is staged, an earlier stage survives), copies the images to pinned
 * memory (they are the caller's again when it returns), queues their generation with the object's current num_want on the stage's own
 * high-priority stream and scratch, into cloud objects nothing else holds, and returns without waiting for the device.  It touches no stream's
 * state and no launch.  One stage per object: a successful call replaces a stage never consumed; cvo_tracks_set_num_want drops the stage;
 * cvo_tracks_reset keeps it (the staged frame is the stream's next frame, whatever its phase then is).
 * cvo_tracks_step_staged_async is cvo_tracks_step_async of the staged list: what depends on the streams' state is checked here.  With nothing
 * staged: CVO_ERR_INVALID.  A step in flight or a listed stream that awaits its decision: CVO_ERR_INVALID, no stream changes and THE STAGE IS KEPT
 * -- commit, then call again.  A staged cloud above 65535 points or a HIP error of the staged work is reported with the code
 * cvo_tracks_step_async returns: no stream changes, the stage is dropped.  Otherwise the call waits on the host only if the staged generation has
 * not finished, hands the staged cloud objects (group boxes made, one launch for all) to the objects' slots, orders its launches behind the
 * stage's stream by an event and queues them: every result is bit-identical to cvo_tracks_step_async on the same frames.
 * cvo_tracks_staged_count: as cvo_batch_staged_count.  cvo_tracks_destroy drains the stage's stream first. */
typedef struct cvo_tracks_s* cvo_tracks;
typedef struct cvo_track_step {
    int phase;                          /* 0, 1, 2: see above */
    int points;                         /* points of the frame's cloud */
    cvo_pair_result  odometry;          /* match_odometry of the frame (phase >= 1) */
    cvo_track_scores odometry_scores;   /* its compute_innerproduct (status CVO_OK only) */
    cvo_pair_result  keyframe;          /* match_keyframe of the frame (phase 2, odometry CVO_OK) */
    cvo_track_scores keyframe_scores;
    float initial_guess[12];            /* what reset_initial returned, cvo.cpp:617 (phase 2, odometry CVO_OK) */
} cvo_track_step;
int cvo_tracks_create(const cvo_params* p /* NULL = defaults */, int device, int max_streams, cvo_tracks* out);
int cvo_tracks_destroy(cvo_tracks t);
int cvo_tracks_set_num_want(cvo_tracks t, int num_want);      /* as cvo_batch_set_num_want (drops staged frames) */
int cvo_tracks_set_arith_mode(cvo_tracks t, int flags);       /* as cvo_batch_set_arith_mode, for both objects' launches */
int cvo_tracks_reset(cvo_tracks t, int s);
int cvo_tracks_step_async(cvo_tracks t, int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                          int width, int height, const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */, void* hip_stream);
int cvo_tracks_stage_async(cvo_tracks t, int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                           int width, int height, const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */);
int cvo_tracks_step_staged_async(cvo_tracks t, void* hip_stream);
int cvo_tracks_staged_count(cvo_tracks t, int* images /* may be NULL */, long long* taken /* may be NULL */);
/* The device twins (see cvo_device_image above for validation and ordering): the step's or the stage's frames read from caller-owned device memory.
 * A refused call changes no stream and keeps the stage.  cvo_tracks_step_staged_async consumes a stage of either kind. */
int cvo_tracks_step_device_async(cvo_tracks t, int count, const int* streams, const cvo_device_image* images, int width, int height,
                                 const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */, void* hip_stream, void* image_stream);
int cvo_tracks_stage_device_async(cvo_tracks t, int count, const int* streams, const cvo_device_image* images, int width, int height,
                                  const cvo_camera* cams, const int* cam_index /* NULL: cams[0] for every image */, void* image_stream);
/* The cloud twin (see cvo_device_cloud above): the step's frames as clouds in caller-owned device memory. */
int cvo_tracks_step_device_clouds_async(cvo_tracks t, int count, const int* streams, const cvo_device_cloud* clouds,
                                        void* hip_stream, void* cloud_stream);
int cvo_tracks_done(cvo_tracks t, int* done);
int cvo_tracks_wait(cvo_tracks t, cvo_track_step* out /* may be NULL */, int count);
int cvo_tracks_commit(cvo_tracks t, int count, const int* streams, const int* accept);
int cvo_tracks_get_cloud(cvo_tracks t, int s, int object, int slot, float* xyz, float* feat, int cap, int* n);
int cvo_tracks_get_selected_points(cvo_tracks t, int s, int object, int slot, unsigned short* px, int cap, int* n);
int cvo_tracks_get_state(cvo_tracks t, int s, int object, float R[9], float T[3], float* ell, float transform[12]);


/* ======================= per-point support: which points of a frame an alignment agrees on (NOT in the reference) ===========
 * function_inner_product (cvo.cpp:388-459) sums the kernel matrix of two clouds into one number; these calls keep it per point.  For clouds a (rows,
 * moved by the 3 x 4 tran_a first when one is given, as cvo.cpp:485-487 does) and b (columns) and a length scale ell, pair (i, j) is INSIDE when
 * d2 < d2_thres and d2_color < d2_c_thres (cvo.cpp:395-396, 423, 428), its value is a_ij = ck * k (cvo.cpp:429-431; no a > sp_thres test, as there), and
 *   sum_a[i]   float  sum over j of a_ij of the inside pairs of row i, added in double in ascending j and rounded once;   count_a[i]  int  how many
 *   sum_b[j]   float  the same over i for column j, ascending i;                                                           count_b[j]  int
 * A point with no inside pair gets 0 and 0 (the "count 0 reads 1" rule of cvo.cpp:455-456 belongs to the cloud's total, not to a point).  The counts
 * of either side add up to the num of cvo_function_inner_product for the same arguments (0 where that reads 1), the sums to its value.  The float
 * sequence is that call's: un-fused d2 (nanoflann.hpp:403-406), double exp, float product; the moved point is computed once and used by both
 * directions, so a_ij is one float on both sides.  Every bit of the four arrays is a function of the two clouds, tran_a, ell and the parameters
 * alone: a row's columns are swept by one lane in ascending order whatever else shares the launch, and nothing is added atomically.  Index i of an
 * array is point i of the cloud, the point cvo_*_get_selected_points maps to its pixel.
 *
 * cvo_point_support: the arguments of cvo_function_inner_product, the handle's ell; writes host arrays and waits.  sum_a and count_a (cap_a entries
 * each) may both be NULL: that direction is not computed; the same for sum_b / count_b.  CVO_ERR_EMPTY_CLOUD for an empty slot, CVO_ERR_INVALID for a
 * cap below the cloud's size, for one array of a direction without the other, and when both directions are NULL: nothing is written then.
 *
 * cvo_batch_point_support: for positions pairs[k] (k < count; NULL: 0 .. count-1) of the LAST launch's list -- the positions cvo_batch_wait reports --
 * a is the pair's moving cloud under the transform, and with the ell, its alignment left in the pair's device-resident state, b its fixed cloud.
 * dst[k] holds that pair's four host arrays (moving: n_moving entries, fixed: n_fixed; a direction's two pointers may both be NULL).  ONE launch for
 * all pairs and both directions, queued behind the align launch on its stream like cvo_batch_enqueue_innerproduct, no transform crosses the host;
 * the call then waits and copies.  It shares no buffer with a score block in flight.  CVO_ERR_INVALID (a position out of range or listed twice, a
 * NULL dst, half a direction, no launch yet, clouds replaced since the launch) and CVO_ERR_EMPTY_CLOUD are found before anything is queued.
 *
 * cvo_batch_point_support_device: the same records pointing into caller-owned DEVICE memory, n x 4 bytes per array, nothing outside them is written.
 * Every pointer is checked before anything is queued by the rule of cvo_device_cloud (device memory of the object's device with the extent inside its
 * allocation, managed, or pinned / registered host memory; pageable host memory: CVO_ERR_INVALID) and must be 4-byte aligned.  Ordering is
 * image_stream's rule with the direction reversed: with an out_stream (a hipStream_t) that stream waits for an event recorded behind the launch and
 * the call returns without a host wait -- work queued on out_stream afterwards sees the arrays, and what out_stream held before the call (a fill of
 * the arrays, their last reader) is waited for by the launch; with NULL the arrays must be idle and the call waits on the host.
 *
 * cvo_tracks_point_support(_device): valid between cvo_tracks_wait of a step and the next cvo_tracks_commit or step.  streams[k] must have been listed
 * in that step, and its `object` (0 odometry, 1 keyframe) must have aligned there with CVO_OK (so: not a phase-0 stream, and object 1 only in phase
 * 2); a is the step's frame at that object's result transform and ell, b that object's fixed cloud.  Anything else: CVO_ERR_INVALID before anything
 * is queued, no stream is touched. */
typedef struct cvo_point_support_dst {
    float* sum_moving; int* count_moving;     /* one entry per point of a (the moving cloud / the step's frame) */
    float* sum_fixed;  int* count_fixed;      /* one entry per point of b (the fixed cloud) */
} cvo_point_support_dst;
int cvo_point_support(cvo_handle h, int slot_a, const float* tran_a /* 3x4 row-major or NULL */, int slot_b,
                      float* sum_a, int* count_a, int cap_a, float* sum_b, int* count_b, int cap_b);
int cvo_batch_point_support(cvo_batch b, int count, const int* pairs /* NULL: 0 .. count-1 */, const cvo_point_support_dst* dst);
int cvo_batch_point_support_device(cvo_batch b, int count, const int* pairs, const cvo_point_support_dst* dst, void* out_stream);
int cvo_tracks_point_support(cvo_tracks t, int object, int count, const int* streams, const cvo_point_support_dst* dst);
int cvo_tracks_point_support_device(cvo_tracks t, int object, int count, const int* streams, const cvo_point_support_dst* dst, void* out_stream);


/* ======================= point matches: each point's best and mean partner under an alignment (NOT in the reference) ===========
 * The per-point support says how much of the energy a point holds; these calls say what the point was matched to.  Rows, columns, the move of a by
 * a transform, the two gates, a_ij = ck * k as one float and no a > sp_thres test are exactly those of "per-point support" above: the moved rows
 * are computed once into a scratch plane both directions read, so a_ij is one float on both sides.  All coordinates below are in the FIXED frame:
 * partners of a moving-side row are points of the fixed cloud as stored, partners of a fixed-side row are the moved moving points.  For every row
 * i of a direction, over the inside pairs of the row:
 *   best[i]          int32    the column j of the largest a_ij, compared as floats; the lowest j on a tie (an ascending sweep with a strict >)
 *   best_value[i]    float    that a_ij
 *   mean[3i..3i+2]   float    (sum_j (double)a_ij * (double)pb_j[q]) / sum_j (double)a_ij, both sums in double in ascending j, the quotient in double,
 *                             rounded to float once: the a-weighted mean of the partners' points
 *   sum[i], count[i]          byte for byte what cvo_*_point_support gives for the same arguments
 * A row with no inside pair gets best = -1 and zeros in every other field.  The arrays are written by the row's own lane, no reduction, no atomics: a
 * row's bits depend on the two clouds, the transform, ell and the parameters alone, not on what else shares the launch.
 *
 * Per direction there is also a fit record, made by a second small kernel (one wave per direction) from what the sweep wrote and the rows' own points:
 *   rows = the direction's rows;  matched = rows with count > 0;  sum_w = sum_i (double)sum[i];  sum_w_res2 = sum_i (double)sum[i] * (double)res2_i,
 *   res2_i in float: r = mean - pa per component, (r0*r0 + r1*r1) + r2*r2, pa the row's point in the fixed frame.  Lane L adds rows L, L + 64, ... in
 *   ascending order, then the 64 lanes are added with a fixed xor-butterfly (32, 16, ..., 1): the record's bits are a function of the arrays alone.
 * Fitness is matched / rows; the weighted RMS residual is sqrt(sum_w_res2 / sum_w) (metres; no matched row: sum_w is 0).
 *
 * The five entry points follow the cvo_*_point_support call of the same name in every respect: the handle form uses the handle's ell, writes host
 * arrays (cap_a / cap_b entries each, mean three times that) and waits; the batch form reads each pair's result transform and ell from its
 * device-resident state behind the last align launch on its stream, ONE sweep launch for all pairs and both directions; the device form checks
 * every pointer by the rule of cvo_device_cloud (4-byte aligned; fit: device memory for two records, 8-byte aligned) and follows the out_stream
 * ordering rule of cvo_batch_point_support_device; the tracks form is valid between cvo_tracks_wait and the next commit or step.  A direction's five
 * arrays are all given or all NULL (not computed; its fit record stays unwritten); both directions NULL is an error.  fit may be NULL.  The errors
 * are those of the support calls, found before anything is queued: nothing is written then.  The calls have buffers of their own: they share none
 * with a score block, a support, seeding or pose-model call in flight, and change no state. */
typedef struct cvo_match_fit { int rows; int matched; double sum_w; double sum_w_res2; } cvo_match_fit;
typedef struct cvo_point_matches_dst {
    int* best_moving; float* best_value_moving; float* mean_moving /* n x 3 */; float* sum_moving; int* count_moving;
    int* best_fixed;  float* best_value_fixed;  float* mean_fixed  /* n x 3 */; float* sum_fixed;  int* count_fixed;
    cvo_match_fit* fit /* [2]: moving, fixed; may be NULL */;
} cvo_point_matches_dst;
int cvo_point_matches(cvo_handle h, int slot_a, const float* tran_a /* 3x4 row-major or NULL */, int slot_b, const cvo_point_matches_dst* dst /* moving = a, fixed = b */,
                      int cap_a, int cap_b);
int cvo_batch_point_matches(cvo_batch b, int count, const int* pairs /* NULL: 0 .. count-1 */, const cvo_point_matches_dst* dst);
int cvo_batch_point_matches_device(cvo_batch b, int count, const int* pairs, const cvo_point_matches_dst* dst, void* out_stream);
int cvo_tracks_point_matches(cvo_tracks t, int object, int count, const int* streams, const cvo_point_matches_dst* dst);
int cvo_tracks_point_matches_device(cvo_tracks t, int object, int count, const int* streams, const cvo_point_matches_dst* dst, void* out_stream);


/* ======================= pose hypotheses: score K start transforms per pair, align from the best (NOT in the reference) ===========
 * The alignment converges from a start that is already close (the radius gate is 10 cm at ell = 0.15).  A loop-closure candidate or a re-localisation
 * has several guesses instead -- detectLoopClousure_top10 holds lc_prior and lc_prior_2 per candidate, aligns from the first and scores both afterwards
 * (keyframe_graph.cpp:649-714; inn_prior, inn_lc_prior in cvo.cpp:539-551).  These calls score the guesses BEFORE the alignment: for each listed pair,
 * k candidate transforms (moving -> fixed, 3x4 row-major, the convention of tran_a in cvo_function_inner_product) and a length scale ell; the score of a
 * hypothesis is cvo_function_inner_product(moving, that transform, fixed) at that ell -- both gates, no a > sp_thres test (cvo.cpp:388-459): value
 * the float of the double sum, num the pair count (1 where it is 0, cvo.cpp:455-456), num_e 0.  All pairs and all hypotheses of a call are ONE launch,
 * a second small one adds up and selects: best = the LOWEST index among the hypotheses with the largest value, compared as floats.
 * The bits of value and num of a (pair, hypothesis) depend on the two clouds, that transform, ell and the parameters alone -- not on k, on the
 * hypothesis' place in the list, on the other pairs of the call or on the launch's shape: a row's columns are swept by one lane in ascending order,
 * the sums are added in a fixed order, nothing atomically.  They agree with cvo_function_inner_product's to the last few bits of a double sum (that
 * kernel cuts the columns into chunks), i.e. to 1e-6 relative in value and exactly in num.
 *
 * cvo_score_hypotheses: scores only, clouds from the handle's slots (a = moving side, b = fixed side), explicit ell; the call waits.  The handle's
 *   R, T, ell and transform are untouched.  best may be NULL.
 * cvo_batch_score_hypotheses: scores only, for batch slots pairs[i] (slot indices as cvo_batch_align_pairs_async takes them; NULL: 0 .. count-1);
 *   a = the slot's moving cloud, b = its fixed cloud; trans holds k transforms per listed slot, in list order.  Takes in a launch in flight first
 *   (as every batch call does), waits and copies.  No state and no start flag of any slot changes: an align launch that follows gives the bits it
 *   would have given without the call.
 * cvo_batch_seed_hypotheses_async: the same two launches on the object's stream, and the select step also writes each listed slot's device-resident
 *   start state: R, T = what cvo_reset_initial(fresh handle, hypothesis[best]) leaves in cvo_get_state (reset_initial with transform = I, cvo.cpp:611-618,
 *   keyframe_graph.cpp:696), ell, transform and iter as cvo_batch_set_pair / cvo_batch_set_state last left them for the slot, everything else zero.
 *   Returns without a host wait; trans has been copied and is the caller's again.  The next align launch that lists a seeded slot starts from that
 *   state -- also on a caller's stream, which is ordered behind the seed by an event -- and its cvo_pair_result is bit-identical to
 *   cvo_batch_set_state(p, R*, T*, ell_p) followed by the same launch, ell_p the slot's own start ell and R*, T* as above.  No score crosses the host.
 *   The seed is DROPPED by anything that makes the slot start from its host-side state again: cvo_batch_set_state (of any slot),
 *   cvo_batch_reset_states, cvo_batch_set_pair, _set_pairs and the other set_pairs_* calls.
 * cvo_batch_hypothesis_results: waits for the last seeding call's two kernels alone (an event of their own, not an align launch queued behind them)
 *   and returns that call's scores (count x k, k that call's) and choices, in its list order.  count above that call's count, or no seeding call
 *   yet: CVO_ERR_INVALID.  Either output may be NULL.
 *
 * Errors, all found before anything is queued, with no output written and no state changed -- CVO_ERR_INVALID: a null pointer (pairs and best aside),
 * k < 1 or k > CVO_MAX_HYPOTHESES, ell not finite or <= 0, a non-finite entry in trans, count < 1 or above the batch's pairs, a slot out of range or
 * listed twice, a stream slot (cvo_batch_advance_*: these carry their own state); CVO_ERR_EMPTY_CLOUD: an empty cloud. */
#define CVO_MAX_HYPOTHESES 64
int cvo_score_hypotheses(cvo_handle h, int slot_a, int slot_b, int k, const float* trans /* k x 12 */, float ell,
                         cvo_inn_p* scores /* k */, int* best /* may be NULL */);
int cvo_batch_score_hypotheses(cvo_batch b, int count, const int* pairs /* slots; NULL: 0 .. count-1 */, int k,
                               const float* trans /* count x k x 12 */, float ell, cvo_inn_p* scores /* count x k */, int* best /* count, may be NULL */);
int cvo_batch_seed_hypotheses_async(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell);
int cvo_batch_hypothesis_results(cvo_batch b, int count, cvo_inn_p* scores /* count x k, may be NULL */, int* best /* count, may be NULL */);


/* ======================= pose models: value, se(3) gradient and Hessian of the inner product at a pose (NOT in the reference) ===========
 * The calls above report the alignment energy at a pose as one number; these say how it changes with the pose.  a is the moving side (rows), b the
 * fixed side (columns), T a 3x4 row-major transform moving -> fixed (the convention of tran_a), ell a length scale.  pa_i = T a_i, computed as the
 * hypotheses' score computes it; pair (i, j) is INSIDE by the two gates of function_inner_product (cvo.cpp:395-396, 423, 428), its value is
 * a_ij = ck * k (cvo.cpp:429-431), no a > sp_thres test: all as in "pose hypotheses".  Define
 *   f(xi) = sum over the inside pairs of a_ij with the moving cloud under Exp(xi^) o T,
 * xi = [omega; v] a twist in the FIXED frame, rotation first, Exp the SE(3) exponential, the inside set held at what it is at xi = 0.  A model:
 *   value   f(0): the float of the double sum              num   the inside pairs, 1 where that is 0 (cvo.cpp:455-456)
 *   grad    df/dxi at 0                                    hess  d2f/dxi2 at 0, 6 x 6 row-major, symmetric bit for bit
 * With il2 = 1 / ell^2 and w_ij = il2 * a_ij (floats), pb = b_j, cr = pa x pb, db = pb - pa:
 *   grad[0..2] = sum w_ij cr      grad[3..5] = sum w_ij db      hess = sum w_ij Blocks_ij + S
 * Blocks: the 21 terms se3_Hessian builds per pair (cvo.cpp:665-704) -- A at (omega, omega), D at (v, v), C at (v, omega), C^T at (omega, v) -- under
 * the weight il2 * ck * k of the energy itself, NOT the reference's il2 * cdot * k (cvo.cpp:662, 707).  S holds 1/2 hat(grad[3..5]) in the (v, omega)
 * block and its transpose in the (omega, v) block, hat(g) = [[0, -g2, g1], [g2, 0, -g0], [-g1, g0, 0]]: the 1/2 omega x v term of Exp.  It vanishes
 * at a stationary pose; with it hess is the exact second derivative (against central differences: 1e-5 of the largest entry, 2e-3 to 1e-2 without).
 * value is MAXIMISED by the alignment: hess is negative definite near a good pose, -hess at a result is an information matrix in the energy's own
 * units, and (-hess) delta = grad is a Newton step, to be applied as Exp(delta^) o T.  cvo_se3_hessian is something else: the reference's matrix
 * (cdot weight, scaled by -1/100000, shifted until every |eigenvalue| >= 1, cvo.cpp:662, 707, 726-748), not the curvature of this energy.
 *
 * Float sequence: a pair's terms are floats, products and sums as written; a row adds its terms to double accumulators in ascending column order, a
 * wave adds its lanes with a fixed butterfly, a second step adds the row blocks in ascending order and then adds S; nothing is added atomically.
 * Every bit of a model depends on the two clouds, T, ell and the parameters alone -- not on k, on the model's place in the call, on the other pairs
 * or on the launch's shape.  value and num are the bytes cvo_score_hypotheses gives for the same arguments.  No inside pair: value 0, num 1, zeros.
 *
 * cvo_pose_models: clouds from the handle's slots (a = moving side, b = fixed side), k transforms, explicit ell; the call waits.  The handle's
 *   state is untouched.
 * cvo_batch_pose_models: for batch slots pairs[i] with the rules of cvo_batch_score_hypotheses (slot indices; NULL: 0 .. count-1; trans holds k
 *   transforms per listed slot, in list order; out count x k).  Takes in a launch in flight first, waits and copies.  No state, seed or start flag
 *   changes: an align launch that follows gives the bytes it would have given without the call.
 * cvo_batch_result_models: for positions pairs[k] (NULL: 0 .. count-1) of the LAST launch's list, with the rules of cvo_batch_point_support: one
 *   model per pair at the transform and ell its alignment left in the pair's device-resident state.  Queued behind the align launch on its stream,
 *   no transform crosses the host; the call then waits and copies.  It shares no buffer with a score block, a support call or a seeding call in
 *   flight.
 *
 * Errors, all found before anything is queued, with nothing written -- cvo_pose_models and cvo_batch_pose_models: those of the hypothesis calls
 * (a null pointer, pairs aside; k < 1 or k > CVO_MAX_HYPOTHESES; ell not finite or <= 0; a non-finite entry in trans; count < 1 or above the batch's
 * pairs; a slot out of range or listed twice; a stream slot: CVO_ERR_INVALID; an empty cloud: CVO_ERR_EMPTY_CLOUD).  cvo_batch_result_models: those
 * of cvo_batch_point_support (a NULL out, no launch yet, count < 1 or above the last launch's, a position out of range or listed twice, clouds
 * replaced since the launch: CVO_ERR_INVALID; CVO_ERR_EMPTY_CLOUD). */
typedef struct cvo_pose_model {
    float  value;     /* f(0): the float of the double sum                                     */
    int    num;       /* inside pairs; 1 where that is 0 (cvo.cpp:455-456)                     */
    double grad[6];   /* df/dxi at 0                                                           */
    double hess[36];  /* d2f/dxi2 at 0, 6 x 6 row-major, symmetric                             */
} cvo_pose_model;
int cvo_pose_models(cvo_handle h, int slot_a, int slot_b, int k, const float* trans /* k x 12 */, float ell, cvo_pose_model* out /* k */);
int cvo_batch_pose_models(cvo_batch b, int count, const int* pairs /* slots; NULL: 0 .. count-1 */, int k,
                          const float* trans /* count x k x 12 */, float ell, cvo_pose_model* out /* count x k */);
int cvo_batch_result_models(cvo_batch b, int count, const int* pairs /* NULL: 0 .. count-1 */, cvo_pose_model* out /* count */);

#ifdef __cplusplus
}
#endif
#endif /* CVO_HIP_H */
