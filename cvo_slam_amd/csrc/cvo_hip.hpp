// cvo_hip.hpp -- dependency-free C++ mirror of the reference's `cvo::cvo` class
// (thirdparty/cvo/include/cvo.hpp:82-282) over the C ABI of include/cvo_hip.h.
//
// Same member names, argument meaning and error behaviour as the reference; Eigen /
// OpenCV types are replaced by plain structs (3x4 row-major transforms, 6x6 row-major
// Hessian) and the RGB / depth images by the cloud pcd_generator would have produced,
// so this header compiles with nothing but a C++11 compiler and libcvo_hip.so.  The
// Eigen/OpenCV drop-in for the real SLAM tree is include/cvo_adaptor.hpp.
#pragma once
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../include/cvo_hip.h"

namespace cvo_hip {

struct Affine3f { float m[12]; Affine3f() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = 1.f; } };
struct Affine3d { double m[12]; Affine3d() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = 1.0; }
                  Affine3f cast_float() const { Affine3f a; for (int i = 0; i < 12; ++i) a.m[i] = (float)m[i]; return a; } };
struct Matrix6d { double m[36]; };

class inn_p {   // cvo.hpp:52-80
public:
    float value; int num; int num_e;
    void copy(const inn_p& r) { value = r.value; num = r.num; num_e = r.num_e; }
    inn_p(float v, int n, int n_e) : value(v), num(n), num_e(n_e) {}
    inn_p() : value(0), num(0), num_e(0) {}
};

class cvo {
    cvo_handle h_ = nullptr;
    void sync() { cvo_get_transform(h_, transform.m); cvo_get_prev_accum_transform(h_, prev_transform.m, accum_transform.m);
                  int i = 0; cvo_get_init(h_, &i); init = i != 0; cvo_get_iteration_number(h_, &iter); }
    static void to(const cvo_inn_p& a, inn_p& b) { b.value = a.value; b.num = a.num; b.num_e = a.num_e; }
public:
    // public members of the reference (cvo.hpp:139-144)
    bool first_frame = true;
    bool init = false;
    int iter = 0;
    Affine3f transform, prev_transform, accum_transform;

    // cvo(const string& calib_file): the calibration only feeds pcd_generator, which is not behind this boundary
    explicit cvo(const std::string& /*calib_file*/ = std::string(), int device = 0) {
        if (cvo_create(nullptr, device, &h_) != CVO_OK) throw std::runtime_error(std::string("cvo_create: ") + cvo_last_error());
    }
    ~cvo() { cvo_destroy(h_); }
    cvo(const cvo&) = delete; cvo& operator=(const cvo&) = delete;

    void set_pcd(const float* xyz, const float* feat, int n) { if (cvo_set_pcd(h_, xyz, feat, n) == CVO_OK) sync(); }

    // "cvo not initialized !" -> print and return, output untouched (cvo.cpp:463-466, 565-568)
    void match_odometry(const float* xyz, const float* feat, int n, Affine3d& transformd) {
        const int rc = cvo_match_odometry(h_, xyz, feat, n, transformd.m);
        if (rc == CVO_ERR_NOT_INITIALIZED) { std::printf("cvo not initialized !\n"); return; }
        if (rc != CVO_OK) throw std::runtime_error(std::string("match_odometry: ") + cvo_last_error());
        sync();
    }
    void match_keyframe(const float* xyz, const float* feat, int n, Affine3d& transformd) {
        const int rc = cvo_match_keyframe(h_, xyz, feat, n, transformd.m);
        if (rc == CVO_ERR_NOT_INITIALIZED) { std::printf("cvo not initialized !\n"); return; }
        if (rc != CVO_OK) throw std::runtime_error(std::string("match_keyframe: ") + cvo_last_error());
        sync();
    }
    // the reference's own signatures take the images (cvo.cpp:345, 461, 563): point-cloud generation on the GPU
    void set_pcd(const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera& cam) {
        if (cvo_set_pcd_images(h_, bgr8, depth16, width, height, &cam) != CVO_OK) throw std::runtime_error(std::string("set_pcd: ") + cvo_last_error());
        sync();
    }
    // not in the reference: the NEXT frame's images, handed over early (cvo_stage_next_frame in include/cvo_hip.h)
    void stage_next_frame(const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera& cam) {
        if (cvo_stage_next_frame(h_, bgr8, depth16, width, height, &cam) != CVO_OK) throw std::runtime_error(std::string("stage_next_frame: ") + cvo_last_error());
    }
    // not in the reference: the arithmetic mode of this object's alignments (cvo_set_arith_mode in include/cvo_hip.h)
    void set_arith_mode(int flags) {
        if (cvo_set_arith_mode(h_, flags) != CVO_OK) throw std::runtime_error(std::string("set_arith_mode: ") + cvo_last_error());
    }
    void match_keyframe(const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera& cam, Affine3d& transformd) {
        const int rc = cvo_match_keyframe_images(h_, bgr8, depth16, width, height, &cam, transformd.m);
        if (rc == CVO_ERR_NOT_INITIALIZED) { std::printf("cvo not initialized !\n"); return; }
        if (rc != CVO_OK) throw std::runtime_error(std::string("match_keyframe: ") + cvo_last_error());
        sync();
    }
    void match_odometry(const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera& cam, Affine3d& transformd) {
        const int rc = cvo_match_odometry_images(h_, bgr8, depth16, width, height, &cam, transformd.m);
        if (rc == CVO_ERR_NOT_INITIALIZED) { std::printf("cvo not initialized !\n"); return; }
        if (rc != CVO_OK) throw std::runtime_error(std::string("match_odometry: ") + cvo_last_error());
        sync();
    }
    // not in the reference: k candidate transforms (moving -> fixed) scored before an alignment, function_inner_product(slot_a moved, slot_b) of each at
    // `ell`; returns the index of the best (cvo_score_hypotheses in include/cvo_hip.h).  The object's R, T, ell and transform are untouched.
    int score_hypotheses(int slot_a, int slot_b, int k, const Affine3f* trans, float ell, inn_p* scores) {
        if (k < 1 || k > CVO_MAX_HYPOTHESES || !trans || !scores) throw std::runtime_error("score_hypotheses: bad argument");
        cvo_inn_p r[CVO_MAX_HYPOTHESES]; float t[CVO_MAX_HYPOTHESES][12]; int best = 0;
        for (int i = 0; i < k; ++i) std::memcpy(t[i], trans[i].m, sizeof(t[i]));
        if (cvo_score_hypotheses(h_, slot_a, slot_b, k, &t[0][0], ell, r, &best) != CVO_OK) throw std::runtime_error(std::string("score_hypotheses: ") + cvo_last_error());
        for (int i = 0; i < k; ++i) to(r[i], scores[i]);
        return best;
    }
    // not in the reference: value, se(3) gradient and Hessian of that inner product at each of k transforms (cvo_pose_models in include/cvo_hip.h)
    void pose_models(int slot_a, int slot_b, int k, const Affine3f* trans, float ell, cvo_pose_model* out) {
        if (k < 1 || k > CVO_MAX_HYPOTHESES || !trans || !out) throw std::runtime_error("pose_models: bad argument");
        float t[CVO_MAX_HYPOTHESES][12];
        for (int i = 0; i < k; ++i) std::memcpy(t[i], trans[i].m, sizeof(t[i]));
        if (cvo_pose_models(h_, slot_a, slot_b, k, &t[0][0], ell, out) != CVO_OK) throw std::runtime_error(std::string("pose_models: ") + cvo_last_error());
    }
    // not in the reference: what each point of slot_a's cloud (moved by tran_a when given; dst's *_moving arrays, cap_a entries) and of slot_b's (*_fixed,
    // cap_b) was matched to, and the directions' fit records (cvo_point_matches in include/cvo_hip.h)
    void point_matches(int slot_a, const Affine3f* tran_a, int slot_b, const cvo_point_matches_dst& dst, int cap_a, int cap_b) {
        if (cvo_point_matches(h_, slot_a, tran_a ? tran_a->m : nullptr, slot_b, &dst, cap_a, cap_b) != CVO_OK) throw std::runtime_error(std::string("point_matches: ") + cvo_last_error());
    }
    void align() { if (cvo_align(h_) != CVO_OK) throw std::runtime_error(std::string("align: ") + cvo_last_error()); sync(); }

    void compute_innerproduct(inn_p& inn_pre, inn_p& inn_post, Matrix6d& post_hessian, Affine3f& tran, int& inliers,
                              inn_p& inn_fixed_pcd, inn_p& inn_moving_pcd, float& cos_angle) {
        cvo_inn_p a, b, c, d;
        if (cvo_compute_innerproduct(h_, &a, &b, post_hessian.m, tran.m, &inliers, &c, &d, &cos_angle) != CVO_OK)
            throw std::runtime_error(std::string("compute_innerproduct: ") + cvo_last_error());
        to(a, inn_pre); to(b, inn_post); to(c, inn_fixed_pcd); to(d, inn_moving_pcd);
    }
    void compute_innerproduct_lc(inn_p& inn_prior, inn_p& inn_lc_prior, inn_p& inn_lc_pre, inn_p& inn_lc_post, Matrix6d& post_hessian,
                                 Affine3f& prior_tran, Affine3f& lc_prior_tran, Affine3f& lc_prior_tran_2, Affine3f& lc_tran,
                                 int& inliers_svd, int& inliers_pnpransac, inn_p& inn_fixed_pcd, inn_p& inn_moving_pcd, float& cos_angle) {
        cvo_inn_p a, b, c, d, e, f;
        if (cvo_compute_innerproduct_lc(h_, &a, &b, &c, &d, post_hessian.m, prior_tran.m, lc_prior_tran.m, lc_prior_tran_2.m, lc_tran.m,
                                        &inliers_svd, &inliers_pnpransac, &e, &f, &cos_angle) != CVO_OK)
            throw std::runtime_error(std::string("compute_innerproduct_lc: ") + cvo_last_error());
        to(a, inn_prior); to(b, inn_lc_prior); to(c, inn_lc_pre); to(d, inn_lc_post); to(e, inn_fixed_pcd); to(f, inn_moving_pcd);
    }

    void update_fixed_pcd() { cvo_update_fixed_pcd(h_); }
    void update_previous_pcd() { cvo_update_previous_pcd(h_); }
    void reset_keyframe(Affine3f& odometry) { cvo_reset_keyframe(h_, odometry.m); sync(); }
    void reset_transform(Affine3f& odometry) { cvo_reset_transform(h_, odometry.m); sync(); }
    Affine3f reset_initial(Affine3f& odometry) { Affine3f out; cvo_reset_initial(h_, odometry.m, out.m); return out; }

    void get_fixed_and_moving_number(int& fixed_num, int& moving_num) { cvo_get_fixed_and_moving_number(h_, &fixed_num, &moving_num); }
    void get_iteration_number(int& iteration) { cvo_get_iteration_number(h_, &iteration); }
    void get_A_nonzero(int& nonzero) { cvo_get_A_nonzero(h_, &nonzero); }
};

// Pose hypotheses for the pairs of a batch (cvo_batch_*_hypotheses in include/cvo_hip.h; not in the reference): k transforms per listed slot, count x k x 12
// floats in list order.  The reference has no batch class, so these are free functions over the C handle; errors throw.
inline void batch_score_hypotheses(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell, cvo_inn_p* scores, int* best = nullptr) {
    if (cvo_batch_score_hypotheses(b, count, pairs, k, trans, ell, scores, best) != CVO_OK) throw std::runtime_error(std::string("batch_score_hypotheses: ") + cvo_last_error());
}
// the same launches, and every listed slot's next alignment starts from its best hypothesis (reset_initial on a fresh object); no host wait
inline void batch_seed_hypotheses_async(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell) {
    if (cvo_batch_seed_hypotheses_async(b, count, pairs, k, trans, ell) != CVO_OK) throw std::runtime_error(std::string("batch_seed_hypotheses_async: ") + cvo_last_error());
}
// the last seeding call's scores and choices; waits for that call's kernels alone
inline void batch_hypothesis_results(cvo_batch b, int count, cvo_inn_p* scores, int* best) {
    if (cvo_batch_hypothesis_results(b, count, scores, best) != CVO_OK) throw std::runtime_error(std::string("batch_hypothesis_results: ") + cvo_last_error());
}

// Pose models for the pairs of a batch (include/cvo_hip.h, "pose models"): k transforms per listed slot, out count x k
inline void batch_pose_models(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell, cvo_pose_model* out) {
    if (cvo_batch_pose_models(b, count, pairs, k, trans, ell, out) != CVO_OK) throw std::runtime_error(std::string("batch_pose_models: ") + cvo_last_error());
}
// one model per listed position of the last launch, at the pair's own result transform and ell
inline void batch_result_models(cvo_batch b, int count, const int* pairs, cvo_pose_model* out) {
    if (cvo_batch_result_models(b, count, pairs, out) != CVO_OK) throw std::runtime_error(std::string("batch_result_models: ") + cvo_last_error());
}

// Point matches for the pairs of a batch (include/cvo_hip.h, "point matches"): one record of host arrays per listed position of the last launch, at the
// pair's own result transform and ell; the device form writes caller-owned device arrays and follows the out_stream ordering rule
inline void batch_point_matches(cvo_batch b, int count, const int* pairs, const cvo_point_matches_dst* dst) {
    if (cvo_batch_point_matches(b, count, pairs, dst) != CVO_OK) throw std::runtime_error(std::string("batch_point_matches: ") + cvo_last_error());
}
inline void batch_point_matches_device(cvo_batch b, int count, const int* pairs, const cvo_point_matches_dst* dst, void* out_stream = nullptr) {
    if (cvo_batch_point_matches_device(b, count, pairs, dst, out_stream) != CVO_OK) throw std::runtime_error(std::string("batch_point_matches_device: ") + cvo_last_error());
}
// K tracker streams (cvo_tracks_* in include/cvo_hip.h): each stream is the pair of objects local_tracker owns, cvo_odometry (object 0) and
// cvo_keyframe (object 1).  Not a class of the reference: there the two objects are stepped one frame, one sequence at a time.  Member names
// follow the C entry points; errors throw, except the statuses a step reports per stream (cvo_track_step).
class CvoTracks {
    cvo_tracks t_ = nullptr;
    static void check(int rc, const char* what) { if (rc != CVO_OK) throw std::runtime_error(std::string(what) + ": " + cvo_last_error()); }
public:
    enum { ODOMETRY = 0, KEYFRAME = 1 };
    explicit CvoTracks(int max_streams, const cvo_params* params = nullptr, int device = 0) { check(cvo_tracks_create(params, device, max_streams, &t_), "cvo_tracks_create"); }
    ~CvoTracks() { cvo_tracks_destroy(t_); }
    CvoTracks(const CvoTracks&) = delete; CvoTracks& operator=(const CvoTracks&) = delete;

    void set_num_want(int num_want) { check(cvo_tracks_set_num_want(t_, num_want), "set_num_want"); }
    void set_arith_mode(int flags) { check(cvo_tracks_set_arith_mode(t_, flags), "set_arith_mode"); }
    void reset(int s) { check(cvo_tracks_reset(t_, s), "reset"); }
    // image k is the next frame of stream streams[k], generated with camera cams[cam_index[k]] (cam_index null: cams[0])
    void step_async(int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                    const cvo_camera* cams, const int* cam_index = nullptr, void* hip_stream = nullptr) {
        check(cvo_tracks_step_async(t_, count, streams, bgr8, depth16, width, height, cams, cam_index, hip_stream), "step_async");
    }
    // the NEXT step's frames, handed over while the current step is in flight (between step_async / step_staged_async and wait); the images are the
    // caller's again when the call returns.  step_staged_async is step_async of the staged list, without generating anything
    void stage_async(int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                     const cvo_camera* cams, const int* cam_index = nullptr) {
        check(cvo_tracks_stage_async(t_, count, streams, bgr8, depth16, width, height, cams, cam_index), "stage_async");
    }
    // the same three for frames in caller-owned device memory (cvo_device_image in include/cvo_hip.h: what is checked, and how image_stream orders
    // the images' writer against the library's ingest; null = already synchronised, the call waits on the host for the ingest alone)
    void step_async(int count, const int* streams, const cvo_device_image* images, int width, int height, const cvo_camera* cams,
                    const int* cam_index = nullptr, void* hip_stream = nullptr, void* image_stream = nullptr) {
        check(cvo_tracks_step_device_async(t_, count, streams, images, width, height, cams, cam_index, hip_stream, image_stream), "step_async");
    }
    void stage_async(int count, const int* streams, const cvo_device_image* images, int width, int height, const cvo_camera* cams,
                     const int* cam_index = nullptr, void* image_stream = nullptr) {
        check(cvo_tracks_stage_device_async(t_, count, streams, images, width, height, cams, cam_index, image_stream), "stage_async");
    }
    void step(int count, const int* streams, const cvo_device_image* images, int width, int height, const cvo_camera* cams, const int* cam_index,
              cvo_track_step* out, void* image_stream = nullptr) {
        step_async(count, streams, images, width, height, cams, cam_index, nullptr, image_stream); wait(out, count);
    }
    void step_staged_async(void* hip_stream = nullptr) { check(cvo_tracks_step_staged_async(t_, hip_stream), "step_staged_async"); }
    int staged_count(long long* taken = nullptr) { int n = 0; check(cvo_tracks_staged_count(t_, &n, taken), "staged_count"); return n; }
    bool done() { int d = 0; check(cvo_tracks_done(t_, &d), "done"); return d != 0; }
    void wait(cvo_track_step* out, int count) { check(cvo_tracks_wait(t_, out, count), "wait"); }
    void step(int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
              const cvo_camera* cams, const int* cam_index, cvo_track_step* out) {
        step_async(count, streams, bgr8, depth16, width, height, cams, cam_index); wait(out, count);
    }
    // the caller's decision for the phase-2 frames just waited for: accept -> update_previous_pcd, else reset_keyframe(t_odometry)
    void commit(int count, const int* streams, const int* accept) { check(cvo_tracks_commit(t_, count, streams, accept), "commit"); }
    int get_cloud(int s, int object, int slot, float* xyz, float* feat, int cap) {
        int n = 0; check(cvo_tracks_get_cloud(t_, s, object, slot, xyz, feat, cap, &n), "get_cloud"); return n;
    }
    int get_selected_points(int s, int object, int slot, unsigned short* px, int cap) {
        int n = 0; check(cvo_tracks_get_selected_points(t_, s, object, slot, px, cap, &n), "get_selected_points"); return n;
    }
    void get_state(int s, int object, float R[9], float T[3], float& ell, Affine3f& transform) {
        check(cvo_tracks_get_state(t_, s, object, R, T, &ell, transform.m), "get_state");
    }
    // point matches of the step just waited for (include/cvo_hip.h, "point matches"): host arrays, or device arrays with the out_stream ordering rule
    void point_matches(int object, int count, const int* streams, const cvo_point_matches_dst* dst) {
        check(cvo_tracks_point_matches(t_, object, count, streams, dst), "point_matches");
    }
    void point_matches_device(int object, int count, const int* streams, const cvo_point_matches_dst* dst, void* out_stream = nullptr) {
        check(cvo_tracks_point_matches_device(t_, object, count, streams, dst, out_stream), "point_matches_device");
    }
};

}  // namespace cvo_hip
