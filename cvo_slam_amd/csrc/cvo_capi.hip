// cvo_capi.hip -- host side of libcvo_hip.so: the C ABI of include/cvo_hip.h.
//
// Holds the state machine of the reference's cvo::cvo object (cloud slots,
// R/T/ell carried between calls, transform bookkeeping; thirdparty/cvo/src/
// cvo.cpp:345-386, 461-618) and drives the gfx950 kernels.  There is no CPU
// compute path: without a gfx950 device every entry point fails with
// CVO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <functional>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cvo_hip.h"
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_queue_classes.hpp"

// what CVO_HIP_QUEUE_CLASSES defaults to (queue_classes(); measured in profiles/hw_queue_classes_ab.txt)
#ifndef CVO_QUEUE_CLASSES_DEFAULT
#define CVO_QUEUE_CLASSES_DEFAULT 1
#endif

// the align kernel's translation unit is in the library four times (cvo_kernels.hip, head comment): cvohip = two waves per SIMD, cvohip_w3 = three;
// cvohip_e337 and cvohip_e337_w3 = the same two with the arithmetic modes (CVO_ARITH_*; the default builds refuse any mode bit)
#define CVO_DECLARE_ALIGN_BUILD(ns) \
namespace ns { \
using cvohip::PairDesc; using cvohip::DevParams; \
size_t align_shared_bytes(int tile, int rows_cap, int y_mode, int y_cap, int tab_cols); \
int align_min_tile(int rows_cap, int y_mode, int y_cap); \
int align_tile_granule(); \
int align_block_max(); \
hipError_t launch_align(int grid, int block, int tile, int rows_cap, int y_mode, int y_cap, int tab_cols, hipStream_t stream, const PairDesc* descs, int n_pairs, int G, \
                        unsigned launch_tag, unsigned long long* queue, const DevParams& P, const unsigned* wgs_submitted, unsigned* wgs_started, const float* const* raw_table, \
                        int arith); \
}
CVO_DECLARE_ALIGN_BUILD(cvohip_e337)
CVO_DECLARE_ALIGN_BUILD(cvohip_e337_w3)
#undef CVO_DECLARE_ALIGN_BUILD
namespace cvohip_w3 {
using cvohip::PairDesc; using cvohip::DevParams;
size_t align_shared_bytes(int tile, int rows_cap, int y_mode, int y_cap, int tab_cols);
int align_min_tile(int rows_cap, int y_mode, int y_cap);
int align_tile_granule();
int align_block_max();
hipError_t launch_align(int grid, int block, int tile, int rows_cap, int y_mode, int y_cap, int tab_cols, hipStream_t stream, const PairDesc* descs, int n_pairs, int G,
                        unsigned launch_tag, unsigned long long* queue, const DevParams& P, const unsigned* wgs_submitted, unsigned* wgs_started, const float* const* raw_table,
                        int arith);
}
namespace cvohip {
size_t align_shared_bytes(int tile, int rows_cap, int y_mode, int y_cap, int tab_cols);
int align_min_tile(int rows_cap, int y_mode, int y_cap);
int align_tile_granule();
int align_blocks_per_cu();
int align_block_max();
hipError_t launch_align(int grid, int block, int tile, int rows_cap, int y_mode, int y_cap, int tab_cols, hipStream_t stream, const PairDesc* descs, int n_pairs, int G,
                        unsigned launch_tag, unsigned long long* queue, const DevParams& P, const unsigned* wgs_submitted, unsigned* wgs_started, const float* const* raw_table,
                        int arith);
int align_adopt_gmax();
hipError_t launch_fill_records(float* rec, int from, int to, int status, hipStream_t stream);
hipError_t launch_copy_records(const float* src, float* dst, int n, hipStream_t stream);
hipError_t launch_pack_clouds(const float* raw, const PackDesc* descs, int n_clouds, int n_max, hipStream_t s);
SelfCacheEntry* score_self_cache(float* gbox, int n);
hipError_t pcd_launch_pyramid(const uint8_t* bgr, int w, int h, float* I0, float* I1, float* I2, float* dx0, float* dy0, float* abs0, float* abs1, float* abs2,
                              int n_img, hipStream_t s);
hipError_t pcd_launch_thresholds(const float* abs0, int w, int h, float* ths, float* ths_smoothed, int n_img, hipStream_t s);
hipError_t pcd_launch_select(const float* abs0, const float* abs1, const float* abs2, const float* ths_smoothed, int w, int h, int pot, uint8_t* map, int* counts,
                             hipStream_t s);
int pcd_tiles(int w, int h);
hipError_t pcd_launch_subsample(uint8_t* map, const uint8_t* pattern, int subsample, int char_th, const uint16_t* depth, int w, int h, int* tile_counts, hipStream_t s);
hipError_t pcd_launch_cloud(const uint8_t* map, const uint16_t* depth, const uint8_t* bgr, const float* dx0, const float* dy0, int w, int h, const float cam[5],
                            const int* tile_counts, int n_points, float* cloud, uint16_t* px, hipStream_t s);
hipError_t pcd_launch_unpack(const float* cloud, int n, float* xyz, float* feat, hipStream_t s);
hipError_t pcd_launch_select_batch(const float* abs0, const float* abs1, const float* abs2, const float* ths_smoothed, int w, int h, uint8_t* map, PcdImgRec* rec,
                                   int n_img, int num_want, hipStream_t s);
hipError_t pcd_launch_subsample_batch(uint8_t* map, const uint8_t* pattern, const PcdImgRec* rec, int num_want, const uint16_t* depth, int w, int h, int* tile_counts,
                                      int n_img, hipStream_t s);
hipError_t pcd_launch_cloud_batch(const uint8_t* map, const uint16_t* depth, const uint8_t* bgr, const float* dx0, const float* dy0, int w, int h, const float cam[5],
                                  const float* cam_table, const int* tile_counts, PcdImgRec* rec, int cap, float* cloud, uint16_t* px, int n_img, hipStream_t s);
hipError_t pcd_launch_scatter(const PcdScatter& S, int n_max, hipStream_t s);
hipError_t pcd_launch_ingest(const PcdIngestDesc* descs, uint8_t* bgr_stack, uint8_t* depth_stack, int w, int h, int n_img, hipStream_t s);
hipError_t launch_ingest_clouds(const CloudIngestDesc* descs, int n_clouds, int n_max, hipStream_t s);
hipError_t launch_reduce_clouds(const ReduceDesc* descs, int n_clouds, int n_max, int slots_max, int rows_max, float voxel, int mode, int min_points,
                                hipStream_t s);
hipError_t launch_count_voxels(const CountDesc* descs, int n_items, int n_max, int slots_max, int min_points, hipStream_t s);
hipError_t launch_reduce_frames(const ReduceDesc* descs, const FrameDesc* frames, int n_frames, int n, int rows_max, float voxel, int mode, int min_points,
                                hipStream_t s);
hipError_t launch_count_frame_voxels(const CountDesc* descs, const FrameDesc* frames, int n_items, int n, int min_points, hipStream_t s);
hipError_t launch_frames_to_clouds(const FrameDesc* frames, const FrameCloudDst* dst, int n_frames, int n, hipStream_t s);
hipError_t launch_fuse_frames(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, const FrameDesc* frames, int n_members, int n, int slots_max,
                              int rows_max, float voxel, int mode, int min_points, int min_views, hipStream_t s);
hipError_t launch_fuse_clouds(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, int n_members, int n_max, int slots_max, int rows_max,
                              float voxel, int mode, int min_points, int min_views, hipStream_t s);
hipError_t launch_view_clouds(const ViewDesc* views, int n_views, int n_max, const ViewParams& P, bool observed, bool images, hipStream_t s);
hipError_t launch_view_maps(const ViewDesc* views, const MapViewSrc* maps, int n_views, int n_max, const ViewParams& P, bool observed, bool images, hipStream_t s);
hipError_t launch_fuse_cells(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, const FrameDesc* frames, int n_members, int n_max, int slots_max,
                             int rows_max, float voxel, hipStream_t s);
hipError_t launch_map_lookup(const MapDesc* maps, int n_maps, const FuseGroupDesc* groups, int n_max, hipStream_t s);
hipError_t launch_map_merge(const MapDesc* maps, int n_maps, const FuseGroupDesc* groups, int cells_max, bool from_map, hipStream_t s);
hipError_t launch_map_extract(const MapDesc* maps, int n_maps, int rows_max, bool write, hipStream_t s);
hipError_t launch_map_compact(const MapDesc* maps, int n_maps, int rows_max, hipStream_t s);
hipError_t launch_map_clear(const void* records, size_t stride, int n_maps, int slots, hipStream_t s);
hipError_t launch_map_merge_cells(const MapMergeDesc* merges, int n_merges, const FuseGroupDesc* groups, int rows_max, hipStream_t s);
hipError_t launch_probe_clouds(const ProbeDesc* probes, int n_probes, int n_max, float voxel, hipStream_t s);
hipError_t launch_probe_frames(const ProbeDesc* probes, const FrameDesc* frames, int n_probes, int n, float voxel, hipStream_t s);
hipError_t launch_map_snapshot(const MapSnapDesc* maps, int n_maps, int rows_max, hipStream_t s);
hipError_t launch_map_restore(const MapSnapDesc* maps, int n_maps, int rows_max, hipStream_t s);
hipError_t launch_map_restore_undo(const MapSnapDesc* maps, int n_maps, int rows_max, int slots, hipStream_t s);
int score_nout();
int score_row_blocks(int na);
int score_groups(int n);
size_t score_box_bytes(int n);
hipError_t launch_cloud_boxes(const float* rec, int n, float* gbox, hipStream_t stream);
hipError_t launch_cloud_boxes_batch(const BoxDesc* descs, int n_clouds, int n_max, hipStream_t stream);
hipError_t launch_adaptive(const AdaptiveArgs& A, int iterations, hipStream_t stream);
int adaptive_partial_records(int nf, int nm);
hipError_t launch_selftest(int kind, const float* in, float* out, int n, hipStream_t s);
hipError_t launch_selftest_reset_initial(const float* in, float* out, int n, hipStream_t s);
hipError_t launch_selftest_voxel_slots(const float* xyz, int n, float voxel, unsigned slots, int* valid, unsigned long long* key, unsigned* slot, hipStream_t s);
hipError_t launch_track_link(const TrackLinkIn* in, const PairState* odo_states, PairState* key_states, TrackLinkOut* out, int n, hipStream_t s);
hipError_t launch_selftest_pairs(const float* in, float* out, float* aux, int n, float ell, const DevParams& P, hipStream_t s);
hipError_t launch_score(const ScoreBatch& B, const ScoreDesc* more, int nreq, int row_blocks, int chunks, const DevParams& P, double* partials,
                        double* out_pinned, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted);
int support_row_blocks(int na);
hipError_t launch_support(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, const SupportDesc* reqs, int n_reqs, int row_blocks,
                          const DevParams& P, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted);
int match_row_blocks(int na);
hipError_t launch_match(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, const MatchDesc* reqs, int n_reqs, int row_blocks,
                        bool with_fit, const DevParams& P, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted);
int hyp_row_blocks(int na);
int hyp_max();
hipError_t launch_hypotheses(const HypDesc* descs, int n_pairs, int k, int row_blocks, const DevParams& P, double* partials, HypScore* scores, int* best,
                             int seed, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted);
int pose_model_row_blocks(int na);
hipError_t launch_pose_models(const PoseModelDesc* descs, int n_pairs, int k, int row_blocks, const DevParams& P, double* partials, PoseModel* out,
                              hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted);
}  // namespace cvohip

using namespace cvohip;

static_assert(sizeof(cvo_trace_row) == sizeof(TraceRow), "trace row layout");
static_assert(sizeof(cvo_adaptive_row) == sizeof(AdaptiveRow), "adaptive trace row layout");
static_assert(sizeof(cvo_inn_p) == sizeof(HypScore), "inn_p record layout");
static_assert(sizeof(cvo_match_fit) == sizeof(MatchFit) && offsetof(cvo_match_fit, sum_w) == offsetof(MatchFit, sum_w) &&
              offsetof(cvo_match_fit, sum_w_res2) == offsetof(MatchFit, sum_w_res2), "match fit record layout");
static_assert(sizeof(cvo_pose_model) == sizeof(PoseModel) && offsetof(cvo_pose_model, grad) == offsetof(PoseModel, grad) &&
              offsetof(cvo_pose_model, hess) == offsetof(PoseModel, hess), "pose model record layout");

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return fail(CVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return CVO_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 4;
        HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return CVO_OK;
    }
    // grow to `need` bytes keeping the first `keep` bytes (copied on `s`, the old block freed when that copy has run)
    int grow_keep(size_t need, size_t keep, hipStream_t s) {
        if (need <= bytes) return CVO_OK;
        void* np = nullptr; const size_t want = need + need / 4;
        HIP_TRY(hipMalloc(&np, want));
        if (p && keep) {
            hipError_t e = hipMemcpyAsync(np, p, std::min(keep, bytes), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { (void)hipFree(np); return fail(CVO_ERR_HIP, std::string("growing a device buffer: ") + hipGetErrorString(e)); }
        }
        if (p) (void)hipFree(p);
        p = np; bytes = want;
        return CVO_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
struct PinBuf {
    void* p = nullptr; size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return CVO_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        HIP_TRY(hipHostMalloc(&p, need + need / 4, hipHostMallocDefault));
        bytes = need + need / 4;
        return CVO_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

// a point cloud resident in HBM: two planes of n float4, {x,y,z,f0} then {f1..f4} (cvo_device.h)
struct Cloud {
    DevBuf buf; int n = 0;
    DevBuf px; int n_px = 0;        // selected pixel (x, y) per point, when the cloud was generated from images
    // boxes of the 32-point groups for the score kernels, made on first use after the points were written
    mutable DevBuf boxes; mutable bool boxes_valid = false; mutable hipStream_t boxes_stream = nullptr;
    // a hand-over the device has not packed yet: the cloud's arrays as they came (n x 3 positions, then 5 channel-major feature arrays) in
    // the engine's pinned staging ring; the next align launch packs them itself, any other consumer runs the pack kernel first
    mutable const float* raw = nullptr;
    mutable const float* raw_feat = nullptr;   // with `raw`: the feature arrays when they do not lie right behind the positions (clouds handed over in caller-registered memory)
    float cost_hint = 0.f;          // mean 1/z^2 of a sample of the points (0 = unknown): what a pair costs per iteration follows the density of its clouds
    bool multi = false;             // held by several slots of one batch (cvo_batch_set_pairs_device_clouds lists a cloud once for several pairs): never written or emptied through a slot
    float* rec() const { return static_cast<float*>(buf.p); }
    ~Cloud() { buf.release(); px.release(); boxes.release(); }
};

// The images a cloud was generated from, as they were staged for the device (pinned host memory): kept after the generation so that a second handle given the
// SAME frame -- the tracker's cvo_odometry and cvo_keyframe objects build their MOVING cloud from one image with a deterministic selector (local_tracker.cpp:356,415;
// SURVEY appendix B) -- can recognise it byte for byte and take a device copy of the finished cloud instead of generating it again (cvo_set_pcd_images).  `stamp`
// is raised before the owner overwrites the buffer: a compare that saw the same stamp before and after has read one image.
struct ImageStage {
    PinBuf buf; std::atomic<unsigned long long> stamp{0};
    std::mutex mu;              // held while the owner rewrites `buf` and while anybody compares against it (the stamp alone would leave memcpy racing memcmp formally)
    ~ImageStage() { buf.release(); }
};
struct LastGenerated {          // per host thread: the handles of one thread are used one after the other, so whoever shares never races with the generator
    std::shared_ptr<ImageStage> stage; unsigned long long stamp = 0;
    int device = -1, w = 0, h = 0, num_want = 0; cvo_camera cam{};
    std::shared_ptr<Cloud> cloud;
};
LastGenerated& last_generated() { static thread_local LastGenerated g; return g; }
struct FrameStager;
FrameStager*& frame_stager_slot() { static thread_local FrameStager* s = nullptr; return s; }
bool share_generated_clouds() { static const bool on = [] { const char* e = std::getenv("CVO_HIP_SHARE_CLOUDS"); return !e || std::atoi(e) != 0; }(); return on; }

// Caller-registered host memory (cvo_host_register): clouds handed over from inside such a range are not copied into the staging ring at all -- the align launch that
// builds their device layout reads them where they are (registered memory is pinned and mapped into the device's address space, like the ring).
struct HostRange { const unsigned char* lo; const unsigned char* hi; };
struct HostRegistry { std::mutex mu; std::vector<HostRange> ranges; };
HostRegistry& host_registry() { static HostRegistry r; return r; }
bool in_registered_memory(const void* p, size_t bytes) {
    HostRegistry& r = host_registry();
    if (r.ranges.empty()) return false;
    std::lock_guard<std::mutex> lk(r.mu);
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (const HostRange& g : r.ranges) if (q >= g.lo && q + bytes <= g.hi) return true;
    return false;
}

// The hand-over's copy into the pinned ring: 12.6 MB per 64-pair step that the host never reads again.  Ordinary stores pull every destination line into the cache first
// (read-for-ownership) and push the caller's data out of it; non-temporal 16-byte stores write the lines straight through (CVO_HIP_UPLOAD_NT=1; off by default: measured, no difference).
inline void ring_copy(void* dst, const void* src, size_t bytes, bool nt) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    if (nt && bytes >= 4096) {
        typedef long long v2di __attribute__((vector_size(16)));
        unsigned char* d = static_cast<unsigned char*>(dst); const unsigned char* s = static_cast<const unsigned char*>(src);
        const size_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
        if (head) { std::memcpy(d, s, head); d += head; s += head; bytes -= head; }
        const size_t body = bytes & ~(size_t)63;
        for (size_t o = 0; o < body; o += 64) {
            v2di a, b, c, e;
            std::memcpy(&a, s + o, 16); std::memcpy(&b, s + o + 16, 16); std::memcpy(&c, s + o + 32, 16); std::memcpy(&e, s + o + 48, 16);
            __builtin_nontemporal_store(a, reinterpret_cast<v2di*>(d + o)); __builtin_nontemporal_store(b, reinterpret_cast<v2di*>(d + o + 16));
            __builtin_nontemporal_store(c, reinterpret_cast<v2di*>(d + o + 32)); __builtin_nontemporal_store(e, reinterpret_cast<v2di*>(d + o + 48));
        }
        if (bytes > body) std::memcpy(d + body, s + body, bytes - body);
        asm volatile("sfence" ::: "memory");
        return;
    }
#endif
    (void)nt;
    std::memcpy(dst, src, bytes);
}

// Copy threads of the hand-over (Engine::upload_many: a batch's host arrays into the pinned ring, 12.6 MB per 64-pair step).  They live as long as the process:
// starting three threads per hand-over cost 0.1 ms of the host's 0.5 per step, and a step's launch is resubmitted that much later (profiles/r04_upload_pool.txt).
class CopyPool {
public:
    static CopyPool& get() { static CopyPool* p = new CopyPool(); return *p; }   // never destroyed: its threads may outlive main()'s statics
    // runs fn(0) .. fn(parts - 1), part 0 on the caller; returns when all are done.  One job at a time (callers queue on the lock).
    template <class F> void run(int parts, F&& fn) {
        if (parts <= 1 || workers_.empty()) { for (int i = 0; i < parts; ++i) fn(i); return; }
        std::unique_lock<std::mutex> job(job_mutex_);
        {
            std::lock_guard<std::mutex> lk(m_);
            task_ = [&fn](int i) { fn(i); }; next_ = 1; parts_ = parts; left_ = parts - 1; ++epoch_;
        }
        cv_.notify_all();
        fn(0);
        for (;;) {                                                    // the caller takes parts too while it waits
            int mine = -1;
            { std::lock_guard<std::mutex> lk(m_); if (next_ < parts_) mine = next_++; }
            if (mine < 0) break;
            fn(mine);
            { std::lock_guard<std::mutex> lk(m_); --left_; }
        }
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return left_ == 0; });
        task_ = nullptr;
    }
private:
    CopyPool() {
        const int hw = (int)std::thread::hardware_concurrency();
        const int n = std::max(0, std::min(7, hw - 1));
        for (int i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
        for (std::thread& t : workers_) t.detach();
    }
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return epoch_ != seen && next_ < parts_; });
            if (next_ >= parts_) { seen = epoch_; continue; }
            const int mine = next_++;
            if (next_ >= parts_) seen = epoch_;
            auto task = task_;
            lk.unlock();
            task(mine);
            lk.lock();
            if (--left_ == 0) done_.notify_all();
        }
    }
    std::mutex m_, job_mutex_;
    std::condition_variable cv_, done_;
    std::function<void(int)> task_;
    int next_ = 0, parts_ = 0, left_ = 0;
    unsigned long long epoch_ = 0;
    std::vector<std::thread> workers_;
};

DevParams to_dev(const cvo_params& p) {
    DevParams d;
    d.sigma = p.sigma; d.sp_thres = p.sp_thres; d.c = p.c; d.d = p.d; d.c_ell = p.c_ell; d.c_sigma = p.c_sigma;
    d.min_step = p.min_step; d.eps = p.eps; d.eps_2 = p.eps_2; d.max_iter = p.max_iter;
    d.skin = 0.25f;
    d.skin_alpha = 0.f; d.alpha_gamma = 0.f; d.first_scale = 1.f; d.fuse_refine = 1;
    d.nt_min = 0;
    d.overlap_stop_test = 1;
    d.predict = 0.7f; d.predict_steps = 8.f;   // lists built / filtered 0.7 of every point's allowance ahead on the path: -10 % culls, +1 % (profiles/r04_predicted_list_centres.txt)
    d.resort = 1;
    d.adopt_kmax = 40; d.adopt_on = 0; d.adopt_inject = 0; d.adopt_dwell = 0;
    d.colocate = 1;
    return d;
}

int check_device(int device, int* num_cus) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(CVO_ERR_NO_DEVICE, "no HIP device visible: libcvo_hip has no CPU path");
    if (device < 0 || device >= count) return fail(CVO_ERR_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CVO_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libcvo_hip is built for gfx950 only");
    if (num_cus) *num_cus = prop.multiProcessorCount;
    return CVO_OK;
}

// Co-residency of cooperating workgroups.  The G > 1 workgroups of a pair wait for each other inside the kernel (tagged granules
// through L2), so all of a launch's workgroups must be resident at the same time.  One launch alone is sized to the CU count, but
// launches of OTHER handles (tracker thread + back-end thread, keyframe_graph.cpp:212-240; a thread pool of loop-closure checks) share
// the CUs: with more cooperating workgroups in flight than the device holds, every launch can end up partially resident and spin until
// the in-kernel timeout.  So the library keeps a book, per device and process-wide, of the cooperative (G > 1) launches in flight and
// the workgroup slots they hold.  A launch that does not fit beside them takes fewer workgroups per pair -- down to G = 1, which waits
// for nobody and needs no slot; results do not depend on G.  When its clouds force G > 1 (more than MAX_ROWS_PER_WG rows per
// workgroup otherwise) it is queued BEHIND the launches in the book instead (hipStreamWaitEvent on their completion events: no host
// thread ever blocks), so it starts on an empty device.  Entries leave the book when their launch has been waited for or the handle
// goes away.  Cooperative launches are submitted under the book's lock (acquire -> kernel launch -> completion event), a few
// microseconds each.  Launches of other processes on the same GPU are outside this book.
struct SlotBook {
    struct Holder { const void* engine; int device; int slots; hipEvent_t done; };
    std::mutex mu;
    std::vector<Holder> holders;
};
SlotBook& slot_book() { static SlotBook b; return b; }

// Adoption (cvo_kernels.hip: finished workgroups help with pairs that still run): a workgroup only offers its help when nothing is
// queued on the device that could start now, i.e. when every workgroup the library has submitted there has started.  Three counters per
// device: submitted (host-written before each launch, pinned host memory the kernels read), started and deferred (device memory, one
// word after the other, bumped by the workgroups).  EVERY align launch of the process counts (with or without adoption, cooperative, queue
// mode), and so does every score launch: those are the kernels whose workgroups wait for a compute unit while persistent align workgroups
// hold them.  A launch adds its grid to `submitted` before it is submitted (and takes it back when the submission fails), and every one of
// its workgroups adds itself to `started` first thing -- except an align launch the host expects to wait behind launches of this library on
// every hardware queue (DevParams::adopt_on, Engine::launch_share): it is not counted as submitted, and its workgroups add themselves to
// `deferred` as well as to `started` when they do start.  Work queued behind a running launch on a shared hardware queue cannot take a
// compute unit before that launch ends, so it must not silence the running launch's helpers.  Healthy paths keep
// submitted + deferred == started whenever nothing counted waits; no host read of the device counters on any healthy path; a launch call
// that reports an error re-synchronises them once the device has drained (resync_adopt_counters).
struct AdoptCounters { int device = -1; unsigned* submitted_host = nullptr; unsigned* submitted_dev = nullptr; unsigned* started_dev = nullptr; };   // started_dev[1]: deferred
AdoptCounters* adopt_counters(int device) {                          // null when they cannot be made: launches then run without adoption
    static std::mutex mu; static std::vector<AdoptCounters*> all;
    std::lock_guard<std::mutex> lk(mu);
    for (AdoptCounters* a : all) if (a->device == device) return a->submitted_host ? a : nullptr;
    AdoptCounters* a = new AdoptCounters; a->device = device;
    void* h = nullptr; void* d = nullptr; void* s = nullptr;
    if (hipHostMalloc(&h, sizeof(unsigned), hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess &&
        hipMalloc(&s, 2 * sizeof(unsigned)) == hipSuccess && hipMemset(s, 0, 2 * sizeof(unsigned)) == hipSuccess) {
        a->submitted_host = static_cast<unsigned*>(h); *a->submitted_host = 0u; a->submitted_dev = static_cast<unsigned*>(d); a->started_dev = static_cast<unsigned*>(s);
    } else { (void)hipGetLastError(); }
    all.push_back(a);
    return a->submitted_host ? a : nullptr;
}
std::mutex& adopt_submit_mutex() { static std::mutex m; return m; }
// A launch call has reported an error.  It may still have been enqueued (hipGetLastError can hand out an earlier, sticky error), so "take the grid back from
// `submitted`" could leave the counters apart for the life of the process -- and the helpers silent (submitted + deferred != started reads "work is queued").  Errors are
// rare: let the device drain and set `submitted` to what has really started and was not deferred.  Called with the submit lock held (nothing counted is submitted meanwhile).
void resync_adopt_counters(AdoptCounters* a) {
    (void)hipDeviceSynchronize();
    unsigned st[2] = {0u, 0u};                                       // started, deferred
    if (hipMemcpy(st, a->started_dev, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess) {
        if (*a->submitted_host + st[1] != st[0])
            std::fprintf(stderr, "cvo_hip: launch error on device %d: adoption counters re-synchronised (submitted %u, deferred %u, started %u)\n", a->device, *a->submitted_host, st[1], st[0]);
        *a->submitted_host = st[0] - st[1];
    }
    (void)hipGetLastError();
}

// Align launches of this library in flight, per device (Engine::launch_share).  Engines register while they live; whether an engine's last launch is
// still on the device is its completion event ev1, recorded under adopt_submit_mutex like the launch itself.  Guarded by adopt_submit_mutex.
std::vector<const struct Engine*>& live_engines() { static std::vector<const Engine*> v; return v; }
// Hardware queues the HIP runtime gives this process: GPU_MAX_HW_QUEUES when set, else the runtime's default of 4.  Read, never set.
int hw_queue_count() {
    static const int q = [] { const char* e = std::getenv("GPU_MAX_HW_QUEUES"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 4; }();
    return q;
}
// Queue classes (cvo_queue_classes.hpp; DESIGN.md section 4.1, "Queue classes"): the runtime's limit of Q hardware queues holds per stream PRIORITY, so the
// streams of batch objects are dealt over two priorities -- class 0 normal, class 1 the least -- and 2 Q of them have a hardware queue each.  The greatest
// priority stays with the stage streams (stage_ready).  CVO_HIP_QUEUE_CLASSES, read once: 0 = every stream normal, 1 = normal then least,
// 2 = normal then greatest (for one measurement: such launches take the queues the staged frames count on).
struct QueueClasses { int mode = 0; std::vector<std::array<int, cvo_qc::CLASSES>> live; };   // live[device][c]: library-made engine streams alive in class c (guarded by adopt_submit_mutex)
QueueClasses& queue_classes() {
    static QueueClasses q = [] { QueueClasses v; const char* e = std::getenv("CVO_HIP_QUEUE_CLASSES"); v.mode = e ? std::max(0, std::min(2, std::atoi(e))) : CVO_QUEUE_CLASSES_DEFAULT; return v; }();
    return q;
}
// the stream priority of class 1 on the current device; false when the device has no such level (or the dealer is off): everything is class 0 then
bool second_class_priority(int* priority) {
    const int mode = queue_classes().mode;
    int least = 0, greatest = 0;
    if (mode == 0 || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); return false; }
    *priority = mode == 2 ? greatest : least;                       // (numerically greater = lower priority; normal is 0)
    return mode == 2 ? greatest < 0 : least > 0;
}

// Launch machinery shared by single-object handles and batches.
struct Engine {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevParams P;
    bool wide_waves = true;          // CVO_HIP_WIDE=0: plane-layout launches run the two-waves-per-SIMD build as well
    bool wide_all = false;           // CVO_HIP_WIDE=2: the float4 layout runs the three-waves-per-SIMD build too (measured again in round 4: profiles/r04_three_waves_tum.txt)
    bool gamma_set = false;          // CVO_HIP_ALPHA_GAMMA given: else the depth-proportional margin falls with ell (gamma 1) in the float4 layout: +1 % (profiles/r04_list_margin_gamma.txt)
    bool alpha_auto = true;          // ... and its depth-proportional part (CVO_HIP_SKIN_ALPHA fixes it; CVO_HIP_SKIN alone = one margin for all rows, alpha 0)
    bool skin_auto = true;           // the list radius margin follows the layout: 0.35 with the cloud resident as 16-byte points (3 k-point shape), 0.30 otherwise -- measured with
                                     // the device full (profiles/r03_skin_sweep.txt): a cull costs LDS and issue time only, a longer list costs memory traffic, and that is dearer
                                     // with 256 workgroups streaming than alone (round 2's 0.25 was tuned on one launch); CVO_HIP_SKIN fixes it
    DevBuf d_descs, d_states, d_ybuf, d_jT, d_ent, d_surv, d_xch, d_queue, d_trace, d_tracelen, d_partials;
    // 64-byte result records, one per pair, written by the align kernel (PairDesc::record); the block a rank contributes to the
    // cross-GPU gather may be longer than its pairs (padding records: pad_from .. pad_to carry pad_status, see padded_records)
    DevBuf d_records;
    int arith = 0;               // CVO_ARITH_* bits of the launches from now on (cvo_set_arith_mode / cvo_batch_set_arith_mode); 0 = the default builds
    int rec_hint = 0;            // records to make room for beyond the pairs of a launch (a batch: its max_pairs + 1)
    int pad_from = 0, pad_to = 0, pad_status = 0;
    PinBuf h_descs, h_states, h_states_in, h_stage, h_partials;   // h_states: final states, written by the kernel itself (mapped pinned memory)
    std::vector<unsigned char> descs_uploaded;                     // what d_descs holds: unchanged descriptors are not sent again
    unsigned launch_seq = 0;
    size_t xch_zeroed_bytes = 0;
    int wg_request = 0;          // 0 = auto
    int tile_request = 0;        // 0 = auto
    int capf_request = 0;        // flat capacity per row (0 = auto)
    int block_request = 0;       // threads per workgroup (0 = auto)
    int per_cu = 1;              // workgroups resident per CU: 1 x 512 threads, or 2 x 256 threads (half the LDS each)
    int max_wgs = 0;             // cap on the workgroups of one launch (0 = none): a share of the device for launches that run side by side
    float last_ms = 0.f;
    bool launched = false;
    int last_G = 1;              // workgroups per pair of the last launch
    bool tail_scores = false;    // align launches also answer the tracker's score block for every pair in the kernel's tail (PairDesc::score_out)
    bool last_tail = false;      // ... and the last launch did
    PinBuf h_tail;               // n x 5 x 24 doubles, written by the kernel
    bool adopt = false;          // finished workgroups help with the pairs of their launch that still run (one workgroup and one slot per pair; CVO_HIP_ADOPT)
    int last_grid = 0, last_helpers = 0, last_concurrent = 0;   // the last align launch: its workgroups, those of them launched as helpers, launch_share's estimate
    bool registered = false;     // in live_engines() (guarded by adopt_submit_mutex)
    int queue_class = 0;         // the priority class of `stream` (queue_classes(); guarded by adopt_submit_mutex once other engines can see this one)
    bool class_counted = false;  // ... and it holds a place in queue_classes().live
    hipStream_t retired_stream = nullptr;   // the class-1 stream this engine left (leave_second_class): kept, idle, until destroy() for whoever still names it
    bool queue_behind = false;   // tracker streams (cvo_tracks_step_async): this engine's launches are queued on a stream that holds other work of the step, which the
                                 // host must not wait for; the engine's own previous launch is what its descriptor table has to be safe from, and that is ev1

    // How much of the device an align launch about to be submitted can count on (called under adopt_submit_mutex).  The HIP runtime maps
    // streams onto Q hardware queues (hw_queue_count) by a rule of its own; launches on one hardware queue run one after the other.
    // So with `inflight` align launches of this library on this device still running or queued (this engine's earlier launch is ahead of
    // this one on its stream and does not count), about concurrent = min(Q, inflight + 1) of them run side by side, each on a share of
    // capacity / concurrent workgroup slots, and when inflight >= Q this one waits behind one of them: deferred.  The limit Q holds per
    // queue class, so the launches are counted per class of their engines (cvo_qc::launch_share).  It is an estimate -- the
    // queue mapping is the runtime's, and launches of other processes are not seen.  When it is wrong, only speed suffers (helpers hold back,
    // or take a compute unit a later launch wanted); results do not depend on it.
    void launch_share(int* concurrent, bool* deferred) {
        std::vector<const Engine*>& live = live_engines();
        if (!registered) { live.push_back(this); registered = true; }
        int inflight[cvo_qc::CLASSES] = {0, 0};
        for (const Engine* o : live) {
            if (o == this || o->device != device || !o->launched) continue;
            const hipError_t e = hipEventQuery(o->ev1);
            if (e == hipErrorNotReady) { ++inflight[o->queue_class]; (void)hipGetLastError(); }
        }
        cvo_qc::launch_share(inflight, queue_class, hw_queue_count(), concurrent, deferred);
    }
    void forget() {
        std::lock_guard<std::mutex> lk(adopt_submit_mutex());
        if (class_counted) { --queue_classes().live[device][queue_class]; class_counted = false; }   // the place in its queue class goes back to the dealer
        if (!registered) return;
        std::vector<const Engine*>& live = live_engines();
        live.erase(std::remove(live.begin(), live.end(), this), live.end());
        registered = false;
    }
    // The engine's own stream, in the queue class the dealer gives it (dealt: a batch object of the public API; everything else is class 0 and counted there).
    int make_stream(bool dealt) {
        int prio = 0;
        const bool second = second_class_priority(&prio);
        {
            std::lock_guard<std::mutex> lk(adopt_submit_mutex());
            auto& live = queue_classes().live;
            if ((int)live.size() <= device) live.resize(device + 1, std::array<int, cvo_qc::CLASSES>{});
            queue_class = cvo_qc::choose_class(live[device].data(), hw_queue_count(), dealt, second);
            ++live[device][queue_class]; class_counted = true;
        }
        if (queue_class == 0) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        else HIP_TRY(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio));
        return CVO_OK;
    }
    // Launches of cooperating workgroups never run below normal priority: the workgroups of a pair wait for each other, and beside a steady supply of normal
    // launches a below-normal one could wait for siblings that never get a compute unit.  A class-1 engine that plans such a launch on its own stream moves
    // to class 0 first, once: its stream drains, a normal stream takes its place wherever the engine names it, the dealer's counts follow.  The old stream
    // stays alive and idle until destroy(): clouds shared with other objects may still name it (Cloud::boxes_stream), and waiting for an idle stream is free.
    int leave_second_class() {
        int prio = 0;
        if (queue_class == 0 || !second_class_priority(&prio) || prio <= 0) return CVO_OK;   // (class 1 above normal, CVO_HIP_QUEUE_CLASSES=2: nothing to fear)
        HIP_TRY(hipStreamSynchronize(stream));
        hipStream_t fresh = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
        {
            std::lock_guard<std::mutex> lk(adopt_submit_mutex());
            auto& live = queue_classes().live[device];
            if (class_counted) { --live[queue_class]; ++live[0]; }
            queue_class = 0;
        }
        for (hipStream_t& r : ring_readers) if (r == stream) r = fresh;
        if (packdesc_stream == stream) packdesc_stream = fresh;
        if (last_stream == stream) last_stream = fresh;
        retired_stream = stream; stream = fresh;
        return CVO_OK;
    }

    void release_slots() {
        SlotBook& b = slot_book();
        std::lock_guard<std::mutex> lk(b.mu);
        for (size_t i = 0; i < b.holders.size();) { if (b.holders[i].engine == this) b.holders.erase(b.holders.begin() + i); else ++i; }
    }
    // How many workgroups per pair this launch may use (<= G_want, >= g_min) given the cooperative launches in flight.  Returns with
    // `lk` locked when the launch is cooperative itself (the caller records its completion event, then unlocks); `wait_for` receives
    // the completion events the launch has to be queued behind when it does not fit beside the launches in the book.
    int acquire_slots(int G_want, int g_min, int n_pairs, std::unique_lock<std::mutex>& lk, std::vector<hipEvent_t>& wait_for) {
        const int capacity = num_cus * per_cu;
        const int share = max_wgs > 0 ? std::min(max_wgs, capacity) : capacity;   // what this launch may take at most
        SlotBook& b = slot_book();
        lk = std::unique_lock<std::mutex>(b.mu);
        for (size_t i = 0; i < b.holders.size();) { if (b.holders[i].engine == this) b.holders.erase(b.holders.begin() + i); else ++i; }   // an earlier launch of this engine precedes this one on its stream
        int used = 0;
        for (const SlotBook::Holder& h : b.holders) if (h.device == device) used += h.slots;
        auto need = [&](int G) { return std::max(1, std::min(n_pairs, share / G)) * G; };
        int G = std::max(G_want, g_min);
        while (G > g_min && G > 1 && need(G) > capacity - used) G /= 2;
        G = std::max(G, g_min);
        if (G <= 1) { lk.unlock(); return 1; }                        // G = 1 waits for nobody: always safe, not in the book
        if (need(G) > capacity - used)                                 // forced cooperative launch on a busy device: run after the others
            for (const SlotBook::Holder& h : b.holders) if (h.device == device) wait_for.push_back(h.done);
        b.holders.push_back(SlotBook::Holder{this, device, need(G), ev1});
        return G;
    }

    int init(int dev, const cvo_params& prm, bool dealt = false) {
        device = dev;
        int rc = check_device(dev, &num_cus); if (rc) return rc;
        HIP_TRY(hipSetDevice(dev));
        if ((rc = make_stream(dealt))) return rc;
        HIP_TRY(hipEventCreate(&ev0)); HIP_TRY(hipEventCreate(&ev1));
        P = to_dev(prm);
        if (const char* e = std::getenv("CVO_HIP_FLAT_CAP")) capf_request = std::atoi(e);
        if (const char* e = std::getenv("CVO_HIP_BLOCK")) block_request = std::atoi(e);
        if (const char* e = std::getenv("CVO_HIP_WGS_PER_CU")) per_cu = std::max(1, std::min(2, std::atoi(e)));
        if (const char* e = std::getenv("CVO_HIP_SKIN")) { P.skin = (float)std::atof(e); skin_auto = false; }
        if (const char* e = std::getenv("CVO_HIP_SKIN_ALPHA")) { P.skin_alpha = std::max(0.f, std::min(0.2f, (float)std::atof(e))); alpha_auto = false; }
        if (const char* e = std::getenv("CVO_HIP_ALPHA_GAMMA")) { P.alpha_gamma = std::max(0.f, std::min(4.f, (float)std::atof(e))); gamma_set = true; }
        if (const char* e = std::getenv("CVO_HIP_FUSE_REFINE")) P.fuse_refine = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_FIRST_SCALE")) { P.first_scale = std::max(0.f, std::min(16.f, (float)std::atof(e))); first_scale_set = true; }
        if (const char* e = std::getenv("CVO_HIP_PREDICT")) P.predict = std::max(0.f, std::min(0.99f, (float)std::atof(e)));
        if (const char* e = std::getenv("CVO_HIP_PREDICT_STEPS")) P.predict_steps = std::max(0.f, (float)std::atof(e));
        if (const char* e = std::getenv("CVO_HIP_OVERLAP_STOP")) P.overlap_stop_test = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_NT_MIN")) P.nt_min = std::max(0, std::atoi(e));
        if (const char* e = std::getenv("CVO_HIP_RESORT")) P.resort = std::max(0, std::min(2, std::atoi(e)));
        if (const char* e = std::getenv("CVO_HIP_COLOCATE")) P.colocate = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_WIDE")) { wide_waves = std::atoi(e) != 0; wide_all = std::atoi(e) >= 2; }
        if (const char* e = std::getenv("CVO_HIP_ADOPT_KMAX")) P.adopt_kmax = std::max(0, std::atoi(e));
        if (const char* e = std::getenv("CVO_HIP_ADOPT_INJECT")) P.adopt_inject = std::atoi(e);
        if (const char* e = std::getenv("CVO_HIP_ADOPT_DWELL_US")) P.adopt_dwell = std::max(0, std::min(100000, std::atoi(e))) * 100;
        if (const char* e = std::getenv("CVO_HIP_ADOPT")) adopt = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_TILE")) tile_request = std::atoi(e);
        if (const char* e = std::getenv("CVO_HIP_WGS")) wg_request = std::atoi(e);
        if (const char* e = std::getenv("CVO_HIP_SELF_CACHE")) self_cache_on = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_UPLOAD_COPY")) upload_copy = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_ORDER_PAIRS")) { order_mode = std::atoi(e); order_pairs = order_mode != 0; }
        if (const char* e = std::getenv("CVO_HIP_INKERNEL_PACK")) inkernel_pack = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_RING_MIRROR")) ring_mirror = std::atoi(e) != 0;
        if (const char* e = std::getenv("CVO_HIP_UPLOAD_THREADS")) upload_threads = std::max(1, std::min(16, std::atoi(e)));
        upload_threads = std::max(1, std::min(upload_threads, (int)std::thread::hardware_concurrency()));
        if (const char* e = std::getenv("CVO_HIP_UPLOAD_NT")) upload_nt = std::atoi(e) != 0;
        return CVO_OK;
    }
    void destroy() {
        forget();                                                    // before ev1 goes: other engines query it
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (last_stream && last_stream != stream) (void)hipStreamSynchronize(last_stream);
        release_slots();
        d_scoredescs.release(); h_scoredescs.release(); h_counts.release();
        for (SideCall* c : {&support_call, &match_call, &hyp_call, &pm_call}) c->release();
        for (DevBuf* b : {&d_bgr, &d_depth, &d_I0, &d_I1, &d_I2, &d_dx0, &d_dy0, &d_abs0, &d_abs1, &d_abs2, &d_ths, &d_thsS, &d_map, &d_pattern, &d_counts, &d_tiles}) b->release();
        for (DevBuf* b : {&d_descs, &d_states, &d_ybuf, &d_jT, &d_ent, &d_surv, &d_xch, &d_queue, &d_trace, &d_tracelen, &d_partials, &d_raw, &d_ring, &d_records}) b->release();
        for (PinBuf* b : {&h_descs, &h_states, &h_states_in, &h_stage, &h_partials, &h_tail, &h_packdesc, &h_rawtab}) b->release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev_ring) (void)hipEventDestroy(ev_ring);
        if (stream) (void)hipStreamDestroy(stream);
        if (retired_stream) (void)hipStreamDestroy(retired_stream);
        stream = retired_stream = nullptr; ev0 = ev1 = nullptr;
    }

    // Host arrays in the reference layout -> the clouds' float4 planes in HBM.  All clouds of one hand-over travel together: their
    // arrays are copied as they are (memcpy, no per-point work on the host) into one block of the pinned staging ring behind a table of
    // PackDesc, ONE host-to-device copy brings block and table over, ONE kernel builds the planes (cvo_pack_clouds_kernel).  The ring
    // is only waited for when it wraps.  Large hand-overs (a batch of 64 pairs = 12.6 MB) are copied into the ring by a few threads.
    struct UploadItem { Cloud* c; const float* xyz; const float* feat; int n; };
    DevBuf d_raw;
    bool first_scale_set = false; float coop_first_scale = 0.f;   // (cvo_batch_create sets the latter)
    int upload_threads = 8;
    bool upload_nt = false;          // measured: no difference in the hand-over loop (profiles/r04_upload_nt_ab.txt) -- the host copy is not what that loop waits for
    bool upload_copy = true;
    bool defer_pack = false;          // batches (cvo_batch_create)
    bool order_pairs = true;          // CVO_HIP_ORDER_PAIRS=0: positions take the pairs in index order
    int order_mode = 1;
    bool inkernel_pack = true;        // CVO_HIP_INKERNEL_PACK=0: deferred clouds always go through the pack kernel
    // Experiment (CVO_HIP_RING_MIRROR=1): a batch's block of the ring is also copied to a device mirror by the copy engine, on the engine's stream, at the hand-over,
    // and the align launch behind it builds the clouds' planes from the mirror instead of reading the pinned ring over PCIe from inside the kernel.  Measured
    // interleaved on one lease: with_host_upload / value 0.928-0.965 on the 20-step command against 0.951-0.959 without, 0.959-0.965 against 0.954-0.957 on the
    // 256-step run: within the run-to-run spread, not kept (profiles/r04_upload_mirror_ab.txt).
    bool ring_mirror = false;
    DevBuf d_ring;                    // device mirror of h_stage (same offsets)
    hipEvent_t ev_ring = nullptr;     // recorded behind the last mirror copy
    std::vector<Cloud*> pending;      // clouds with a hand-over not packed yet (Cloud::raw)
    PinBuf h_packdesc, h_rawtab;
    hipStream_t packdesc_stream = nullptr;
    std::vector<hipStream_t> ring_readers;   // every stream with work queued that reads the staging ring (pack kernels, launches that pull raw clouds): all of them before the ring is written over
    void add_ring_reader(hipStream_t s) { if (std::find(ring_readers.begin(), ring_readers.end(), s) == ring_readers.end()) ring_readers.push_back(s); }
    int sync_ring_readers() {
        for (hipStream_t r : ring_readers) if (r != stream) HIP_TRY(hipStreamSynchronize(r));
        ring_readers.clear();
        return CVO_OK;
    }
    // pack kernel over every pending cloud, on stream s (zero-copy from the ring)
    int flush_pending(hipStream_t s) {
        if (pending.empty()) return CVO_OK;
        if (packdesc_stream) { HIP_TRY(hipStreamSynchronize(packdesc_stream)); packdesc_stream = nullptr; }   // an earlier flush may still read the table
        int rc = h_packdesc.ensure(sizeof(PackDesc) * pending.size()); if (rc) return rc;
        PackDesc* pd = static_cast<PackDesc*>(h_packdesc.p);
        const float* base = static_cast<const float*>(h_stage.p);
        int n_max = 0, q = 0;
        for (Cloud* c : pending) {
            if (!c->raw || c->n <= 0) { c->raw = nullptr; continue; }
            pd[q].raw_off = (unsigned long long)(c->raw - base); pd[q].dst = c->rec(); pd[q].n = c->n; pd[q].pad_ = 0;   // (a cloud in registered memory: the difference wraps, base + it is the cloud again)
            pd[q].feat_off = c->raw_feat ? (unsigned long long)(c->raw_feat - base) : 0ull; ++q;
            n_max = std::max(n_max, c->n); c->raw = nullptr; c->raw_feat = nullptr;
        }
        pending.clear();
        if (q == 0) return CVO_OK;
        const hipError_t e = launch_pack_clouds(base, pd, q, n_max, s);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("cloud pack kernel launch: ") + hipGetErrorString(e));
        packdesc_stream = s; add_ring_reader(s);
        return CVO_OK;
    }
    // before the ring is written over: nothing may still have to read it
    int drain_ring() {
        // a launch of this engine on a caller's stream may still read the clouds the pack kernel below writes, or pull clouds from the ring itself
        if (launched && last_stream && last_stream != stream) HIP_TRY(hipStreamSynchronize(last_stream));
        int rc = flush_pending(stream); if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        return sync_ring_readers();
    }
    int upload_many(const UploadItem* it, int count) {
        HIP_TRY(hipSetDevice(device));
        int live = 0, n_max = 0; size_t raw_floats = 0;
        for (int k = 0; k < count; ++k) {
            if (!it[k].c) return fail(CVO_ERR_INVALID, "null cloud");
            if (it[k].n < 0) return fail(CVO_ERR_INVALID, "negative point count");
            if (it[k].n > 65535) return fail(CVO_ERR_INVALID, "more than 65535 points per cloud is not supported (16-bit column indices)");
            if (it[k].n > 0 && (!it[k].xyz || !it[k].feat)) return fail(CVO_ERR_INVALID, "null cloud pointer");
            if (it[k].n > 0) { ++live; n_max = std::max(n_max, it[k].n); raw_floats += (size_t)it[k].n * REC; }
        }
        for (int k = 0; k < count; ++k) {
            Cloud& c = *it[k].c;
            c.n = it[k].n; c.boxes_valid = false; c.cost_hint = 0.f;
            if (c.n > 0) { int rc = c.buf.ensure((size_t)c.n * REC * sizeof(float)); if (rc) return rc; }
            if (c.n > 0) {                                          // every 16th point: enough to rank the pairs of a batch (launch_impl)
                double acc = 0; int m = 0;
                for (int i = 0; i < c.n; i += 16) { const float z = it[k].xyz[(size_t)i * 3 + 2]; if (z > 1e-3f) { acc += 1.0 / ((double)z * z); ++m; } }
                c.cost_hint = m ? (float)(acc / m) : 0.f;
            }
        }
        uploads_pending = true;
        if (live == 0) return CVO_OK;
        const size_t desc_bytes = (sizeof(PackDesc) * (size_t)live + 255) & ~(size_t)255;
        const size_t bytes = desc_bytes + raw_floats * sizeof(float);
        const size_t want = std::max(bytes, (size_t)16 << 20);
        int rc;
        if (h_stage.bytes < want) {
            rc = drain_ring(); if (rc) return rc;                    // the old buffer may still feed a copy or a kernel
            rc = h_stage.ensure(want); if (rc) return rc;
            stage_used = 0;
        }
        if (stage_used + bytes > h_stage.bytes) { rc = drain_ring(); if (rc) return rc; stage_used = 0; }
        if (!defer_pack && upload_copy && d_raw.bytes < bytes) { HIP_TRY(hipStreamSynchronize(stream)); rc = d_raw.ensure(bytes); if (rc) return rc; }   // an earlier pack kernel may still read it
        unsigned char* blk = static_cast<unsigned char*>(h_stage.p) + stage_used;
        stage_used += (bytes + 255) & ~(size_t)255;
        PackDesc* pd = reinterpret_cast<PackDesc*>(blk);             // (read by the pack kernel of the single-object path below; a batch's table is made by flush_pending)
        float* raw = reinterpret_cast<float*>(blk + desc_bytes);
        struct Piece { const float* src; float* dst; size_t bytes; };
        std::vector<Piece> pieces; pieces.reserve(2 * (size_t)live);
        size_t off = 0; int q = 0;
        std::vector<char> in_place(count, 0);                          // clouds of a batch that lie in caller-registered memory: read where they are
        for (int k = 0; k < count; ++k) {
            const int n = it[k].n; if (n <= 0) continue;
            in_place[k] = defer_pack && inkernel_pack && !ring_mirror && in_registered_memory(it[k].xyz, sizeof(float) * 3 * (size_t)n) && in_registered_memory(it[k].feat, sizeof(float) * 5 * (size_t)n);
            pd[q].raw_off = off; pd[q].dst = it[k].c->rec(); pd[q].n = n; pd[q].pad_ = 0; pd[q].feat_off = 0; ++q;
            if (!in_place[k]) {
                pieces.push_back(Piece{it[k].xyz, raw + off, sizeof(float) * 3 * (size_t)n});
                pieces.push_back(Piece{it[k].feat, raw + off + 3 * (size_t)n, sizeof(float) * 5 * (size_t)n});
            }
            off += (size_t)n * REC;
        }
        const int nthreads = (bytes >= ((size_t)2 << 20) && !pieces.empty()) ? std::max(1, std::min(upload_threads, (int)pieces.size())) : 1;
        const bool nt = upload_nt && defer_pack;                     // (a single object's block is copied on by the DMA engine right away: let it come from the cache)
        auto copy_range = [&pieces, nt](size_t a, size_t b) { for (size_t i = a; i < b; ++i) ring_copy(pieces[i].dst, pieces[i].src, pieces[i].bytes, nt); };
        if (nthreads == 1) copy_range(0, pieces.size());
        else {                                                        // in 4 x nthreads parts, taken by the pool's threads and the caller as they come free
            const int parts = std::min((int)pieces.size(), 4 * nthreads);
            const size_t per = (pieces.size() + parts - 1) / parts;
            CopyPool::get().run(parts, [&](int t) { copy_range(std::min(pieces.size(), (size_t)t * per), std::min(pieces.size(), (size_t)(t + 1) * per)); });
        }
        // Batches: the clouds stay in the ring as they came; the next align launch packs each pair's clouds itself, reading the ring where
        // it lies (pinned host memory is mapped into the device's address space): no copy-engine transfer and no kernel of its own between
        // the hand-over and the launch -- both cost a tenth of the throughput beside eight persistent launches (copies of different streams
        // share the DMA engines, small kernels wait for a compute unit no persistent workgroup occupies).  Anything else that wants the
        // clouds first (a score block, a cooperative launch) runs the pack kernel on them (flush_pending).
        if (defer_pack) {
            if (ring_mirror && inkernel_pack) {
                if (d_ring.bytes < h_stage.bytes) { HIP_TRY(hipStreamSynchronize(stream)); for (hipStream_t r : ring_readers) if (r != stream) HIP_TRY(hipStreamSynchronize(r)); rc = d_ring.ensure(h_stage.bytes); if (rc) return rc; }
                HIP_TRY(hipMemcpyAsync(static_cast<unsigned char*>(d_ring.p) + (blk - static_cast<unsigned char*>(h_stage.p)), blk, bytes, hipMemcpyHostToDevice, stream));
                if (!ev_ring) HIP_TRY(hipEventCreateWithFlags(&ev_ring, hipEventDisableTiming));
                HIP_TRY(hipEventRecord(ev_ring, stream));
            }
            size_t o2 = 0;
            for (int k = 0; k < count; ++k) {
                const int n = it[k].n; if (n <= 0) continue;
                if (!it[k].c->raw) pending.push_back(it[k].c);
                if (in_place[k]) { it[k].c->raw = it[k].xyz; it[k].c->raw_feat = it[k].feat; }
                else { it[k].c->raw = raw + o2; it[k].c->raw_feat = nullptr; }
                o2 += (size_t)n * REC;
            }
            return CVO_OK;
        }
        // Single objects: one host-to-device copy of the block, one pack kernel.  (CVO_HIP_UPLOAD_COPY=0: the kernel reads the ring itself.)
        const unsigned char* src = blk;
        if (upload_copy) {
            HIP_TRY(hipMemcpyAsync(d_raw.p, blk, bytes, hipMemcpyHostToDevice, stream));
            src = static_cast<const unsigned char*>(d_raw.p);
        }
        const hipError_t e = launch_pack_clouds(reinterpret_cast<const float*>(src + desc_bytes), reinterpret_cast<const PackDesc*>(src), live, n_max, stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("cloud pack kernel launch: ") + hipGetErrorString(e));
        return CVO_OK;
    }
    int upload(Cloud& c, const float* xyz, const float* feat, int n) {
        const UploadItem it{&c, xyz, feat, n};
        return upload_many(&it, 1);
    }

    // ---- pcd_generator on the GPU (cvo_pcd_kernels.hip).  Image-sized scratch lives with the engine.
    DevBuf d_bgr, d_depth, d_I0, d_I1, d_I2, d_dx0, d_dy0, d_abs0, d_abs1, d_abs2, d_ths, d_thsS, d_map, d_pattern, d_counts, d_tiles;
    PinBuf h_counts;
    std::shared_ptr<ImageStage> img_stage;                          // the frame's images as staged for the copy to the device (ImageStage above)
    int pattern_len = 0;
    // glibc srand(seed); rand() & 0xFF, n times (PixelSelector2.cpp:36-38): TYPE_3 additive feedback generator
    static void rand_pattern(unsigned seed, unsigned char* out, size_t n) {
        std::vector<uint32_t> r(344 + n);
        r[0] = seed ? seed : 1;
        for (int i = 1; i < 31; ++i) {
            const long long hi = (int32_t)r[i - 1] / 127773, lo = (int32_t)r[i - 1] % 127773;
            long long word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            r[i] = (uint32_t)word;
        }
        for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
        for (size_t i = 34; i < 344 + n; ++i) r[i] = r[i - 31] + r[i - 3];
        for (size_t k = 0; k < n; ++k) out[k] = (unsigned char)((r[344 + k] >> 1) & 0xFF);
    }
    int generate_pcd(Cloud& c, const unsigned char* bgr8, const unsigned short* depth16, int w, int h, const cvo_camera& cam, int num_want) {
        HIP_TRY(hipSetDevice(device));
        static const bool timing = std::getenv("CVO_HIP_PCD_TIMING") != nullptr;   // development aid: where a generation's host time goes (stderr)
        const auto tq0 = std::chrono::steady_clock::now(); auto tq = tq0; double tms[6] = {0, 0, 0, 0, 0, 0}; int tqi = 0;
        auto lap = [&]() { if (timing && tqi < 6) { const auto now = std::chrono::steady_clock::now(); tms[tqi++] = std::chrono::duration<double, std::micro>(now - tq).count(); tq = now; } };
        if (!bgr8 || !depth16) return fail(CVO_ERR_INVALID, "null image pointer");
        if (w < 64 || h < 64 || (size_t)w * h > (size_t)1 << 26) return fail(CVO_ERR_INVALID, "image size out of range");
        if (num_want <= 0) return fail(CVO_ERR_INVALID, "num_want must be positive");
        const size_t n = (size_t)w * h;
        const int w1 = w / 2, h1 = h / 2, w2 = w1 / 2, h2 = h1 / 2, w32 = w / 32, h32 = h / 32;
        int rc;
        if ((rc = d_bgr.ensure(3 * n))) return rc;
        if ((rc = d_depth.ensure(2 * n))) return rc;
        for (DevBuf* b : {&d_I0, &d_dx0, &d_dy0, &d_abs0}) if ((rc = b->ensure(sizeof(float) * n))) return rc;
        for (DevBuf* b : {&d_I1, &d_abs1}) if ((rc = b->ensure(sizeof(float) * (size_t)w1 * h1))) return rc;
        for (DevBuf* b : {&d_I2, &d_abs2}) if ((rc = b->ensure(sizeof(float) * (size_t)w2 * h2))) return rc;
        const size_t nths = (size_t)w32 * h32 + 100;                    // +100 zeroed slack, read for rows past h/32 (PixelSelector2.cpp:44-45)
        if ((rc = d_ths.ensure(sizeof(float) * nths))) return rc;
        if ((rc = d_thsS.ensure(sizeof(float) * nths))) return rc;
        if ((rc = d_map.ensure(n))) return rc;
        if ((rc = d_counts.ensure(sizeof(int) * 8))) return rc;
        if ((rc = h_counts.ensure(sizeof(int) * 8))) return rc;
        if (!img_stage) img_stage = std::make_shared<ImageStage>();     // (the copies of the previous generation have run: it ended with a synchronize)
        img_stage->stamp.fetch_add(1, std::memory_order_acq_rel);       // whoever compares against the old content sees that it is going
        if ((rc = img_stage->buf.ensure(5 * n))) return rc;
        if (pattern_len != (int)n) {                                    // the byte pattern only depends on w*h: made once
            if ((rc = d_pattern.ensure(n))) return rc;
            std::vector<unsigned char> pat(n);
            rand_pattern(3141592u, pat.data(), n);
            HIP_TRY(hipMemcpy(d_pattern.p, pat.data(), n, hipMemcpyHostToDevice));
            pattern_len = (int)n;
        }
        unsigned char* st = static_cast<unsigned char*>(img_stage->buf.p);
        // every return from here on leaves nothing of this call in flight: the next generation overwrites the pinned stage the copies read from
        struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{stream};
        std::unique_lock<std::mutex> stage_lock(img_stage->mu);
        // the colour image first: its copy and the gradient / threshold kernels (which need nothing else) run while the host stages the depth image
        std::memcpy(st, bgr8, 3 * n);
        HIP_TRY(hipMemcpyAsync(d_bgr.p, st, 3 * n, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_ths.p, 0, sizeof(float) * nths, stream));
        HIP_TRY(hipMemsetAsync(d_thsS.p, 0, sizeof(float) * nths, stream));
        float* I0 = (float*)d_I0.p; float* dx0 = (float*)d_dx0.p; float* dy0 = (float*)d_dy0.p; float* abs0 = (float*)d_abs0.p;
        hipError_t e = pcd_launch_pyramid((const uint8_t*)d_bgr.p, w, h, I0, (float*)d_I1.p, (float*)d_I2.p, dx0, dy0, abs0, (float*)d_abs1.p, (float*)d_abs2.p, 1, stream);
        if (e == hipSuccess) e = pcd_launch_thresholds(abs0, w, h, (float*)d_ths.p, (float*)d_thsS.p, 1, stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd kernels: ") + hipGetErrorString(e));
        lap();                                                          // [0] buffers, colour staging + copy + kernels queued
        std::memcpy(st + 3 * n, depth16, 2 * n);
        stage_lock.unlock();
        HIP_TRY(hipMemcpyAsync(d_depth.p, st + 3 * n, 2 * n, hipMemcpyHostToDevice, stream));
        lap();                                                          // [1] depth staging + copy queued
        // PixelSelector::makeMaps (PixelSelector2.cpp:136-282), a fresh selector per frame: potential 3, one re-selection allowed
        int pot = 3, recursions_left = 1, ideal = 3;
        float num_have = 0, quotia = 0;
        const float num_want_f = (float)num_want;
        int* hc = static_cast<int*>(h_counts.p);
        for (;;) {
            HIP_TRY(hipMemsetAsync(d_map.p, 0, n, stream));
            HIP_TRY(hipMemsetAsync(d_counts.p, 0, sizeof(int) * 8, stream));
            e = pcd_launch_select(abs0, (const float*)d_abs1.p, (const float*)d_abs2.p, (const float*)d_thsS.p, w, h, pot, (uint8_t*)d_map.p, (int*)d_counts.p, stream);
            if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd select: ") + hipGetErrorString(e));
            HIP_TRY(hipMemcpyAsync(hc, d_counts.p, sizeof(int) * 3, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            lap();                                                      // [2] (and [3] after a re-selection) everything up to the selection's counts
            num_have = (float)(hc[0] + hc[1] + hc[2]);                  // :191
            quotia = num_want_f / num_have;                             // :192
            const float K = num_have * (pot + 1) * (pot + 1);           // :195
            ideal = (int)(sqrtf(K / num_want_f) - 1);                   // :196
            if (ideal < 1) ideal = 1;
            if (recursions_left > 0 && quotia > 1.25 && pot > 1) {      // :199-213
                if (ideal >= pot) ideal = pot - 1;
                pot = ideal; --recursions_left; continue;
            }
            if (recursions_left > 0 && quotia < 0.25) {                 // :214-229
                if (ideal <= pot) ideal = pot + 1;
                pot = ideal; --recursions_left; continue;
            }
            break;
        }
        const int subsample = (quotia < 0.95) ? 1 : 0;                  // :252-268
        const int char_th = subsample ? (int)(unsigned char)(255 * quotia) : 255;
        const float camv[5] = {cam.scaling_factor, cam.fx, cam.fy, cam.cx, cam.cy};
        const int nt = pcd_tiles(w, h);
        if ((rc = d_tiles.ensure(sizeof(int) * 3 * (size_t)nt))) return rc;
        if ((rc = h_counts.ensure(sizeof(int) * std::max(8, 3 * nt)))) return rc;
        hc = static_cast<int*>(h_counts.p);
        e = pcd_launch_subsample((uint8_t*)d_map.p, (const uint8_t*)d_pattern.p, subsample, char_th, (const uint16_t*)d_depth.p, w, h, (int*)d_tiles.p, stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd sub-sampling: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(hc, d_tiles.p, sizeof(int) * 3 * (size_t)nt, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        lap();                                                          // sub-sampling + tile counts
        int npts = 0;
        for (int t = 0; t < nt; ++t) npts += hc[nt + t];                 // kept pixels with a valid depth = points (pcd_generator.cpp:471)
        if (npts > 65535) return fail(CVO_ERR_INVALID, "more than 65535 points per cloud is not supported (16-bit column indices)");
        c.n = npts; c.n_px = npts; c.boxes_valid = false;
        if (npts == 0) return CVO_OK;
        if ((rc = c.buf.ensure((size_t)npts * REC * sizeof(float)))) return rc;
        if ((rc = c.px.ensure((size_t)npts * 2 * sizeof(uint16_t)))) return rc;
        e = pcd_launch_cloud((const uint8_t*)d_map.p, (const uint16_t*)d_depth.p, (const uint8_t*)d_bgr.p, dx0, dy0, w, h, camv, (const int*)d_tiles.p, npts, c.rec(),
                             (uint16_t*)c.px.p, stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd cloud: ") + hipGetErrorString(e));
        HIP_TRY(hipStreamSynchronize(stream));
        lap();                                                          // the cloud itself
        if (timing) std::fprintf(stderr, "[cvo_hip] generate_pcd laps (us): %.0f %.0f %.0f %.0f %.0f %.0f, total %.0f\n", tms[0], tms[1], tms[2], tms[3], tms[4], tms[5],
                                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tq0).count());
        return CVO_OK;
    }

    struct PairIn { const Cloud* fixed; const Cloud* moving; };

    int pick_workgroups(int n_pairs, int nf_max) const {
        int G = wg_request;
        if (G <= 0) {
            // lowest latency of this launch alone: as many workgroups per pair as the CUs allow, but not below ~384 rows per
            // workgroup -- a row's list is walked by one lane, so beyond one 64-row block per wave nothing gets shorter while the
            // partial-sum exchanges keep costing (measured at 3072 points: 2.37 ms at 4, 2.33 at 8, 2.44 at 16, 2.78 at 32, 4.9 at 1)
            // (round 5: at most ~384 rows per workgroup, not at least -- a cloud of 2 817 points, what the generator makes of a 640 x 480 frame, took 4 workgroups
            // of 704 rows where 8 of 352 align it in 1.20 ms instead of 1.37: scripts/r05/probe_tracker_g.py)
            const int rows_max = 384 * (align_block_max() / 512);
            const int want = std::max(1, std::min(32, (nf_max + rows_max - 1) / rows_max));
            G = 1; while (G * 2 * n_pairs <= num_cus * per_cu && G < want) G *= 2;
        }
        const int g_min = (((nf_max + 127) / 128) + (MAX_ROWS_PER_WG / 128) - 1) / (MAX_ROWS_PER_WG / 128);   // a workgroup owns at most MAX_ROWS_PER_WG rows, dealt in blocks of 128
        G = std::max(std::max(1, g_min), std::min(G, num_cus));
        return G;
    }

    // One persistent launch aligning n pairs.  states (host, n entries) are uploaded
    // first when upload_states is set; results land in h_states after wait().
    // state_index (may be null = position i): the device state a position starts from and writes back, d_states[state_index[i]] -- a batch
    // keeps one per pair slot, whichever launch positions its pairs take.  upload_each (may be null = upload_states for every position):
    // position i starts from states_in[i] instead of its device state.
    int state_slots = 0;              // device states kept (at least the launch's pairs): a batch's max_pairs
    int launch(const std::vector<PairIn>& pairs, const PairState* states_in, bool upload_states, hipStream_t on_stream,
               bool want_trace, int trace_cap, const int* state_index = nullptr, const unsigned char* upload_each = nullptr) {
        const int rc = launch_impl(pairs, states_in, upload_states, on_stream, want_trace, trace_cap, state_index, upload_each);
        if (rc != CVO_OK) release_slots();                            // nothing of this call is on the device
        return rc;
    }
    int launch_impl(const std::vector<PairIn>& pairs, const PairState* states_in, bool upload_states, hipStream_t on_stream,
                    bool want_trace, int trace_cap, const int* state_index, const unsigned char* upload_each) {
        HIP_TRY(hipSetDevice(device));
        const int n = (int)pairs.size();
        if (n <= 0) return fail(CVO_ERR_INVALID, "no pairs to align");
        int nf_max = 0, nm_max = 0;
        for (const PairIn& p : pairs) { nf_max = std::max(nf_max, p.fixed ? p.fixed->n : 0); nm_max = std::max(nm_max, p.moving ? p.moving->n : 0); }
        if (queue_class != 0 && !on_stream && pick_workgroups(n, nf_max) > 1) { int rcq = leave_second_class(); if (rcq) return rcq; }   // (before the stream is named below)
        hipStream_t s = on_stream ? on_stream : stream;
        { int rcs = settle_uploads(s); if (rcs) return rcs; }
        const int g_floor = std::max(1, (((nf_max + 127) / 128) + (MAX_ROWS_PER_WG / 128) - 1) / (MAX_ROWS_PER_WG / 128));
        std::unique_lock<std::mutex> book_lock; std::vector<hipEvent_t> run_after;
        const int G = acquire_slots(pick_workgroups(n, nf_max), g_floor, n, book_lock, run_after);   // fewer workgroups per pair beside other handles' cooperative launches
        last_G = G;
        const int slots = std::max(1, std::min(n, (max_wgs > 0 ? std::min(max_wgs, num_cus * per_cu) : num_cus * per_cu) / G));   // every workgroup of the grid must be resident
        const int grid = slots * G;
        const int nf_pad = round_up(std::max(nf_max, 1), 64), nm_pad = round_up(std::max(nm_max, 1), 64);
        int capf = capf_request;
        // room for the nonzero records: nm/6 per row on average (512 at 3 k points; a fronto-parallel wall half a metre from the
        // camera gives ~300 neighbours per row at the first ell), beyond that the dense per-row fallback takes over
        if (capf <= 0) capf = std::max(128, nm_max / 6);
        // Which build of the kernel runs the launch, and its LDS plan.  Clouds that only fit in the plane layout (9 k points) run with three waves per SIMD:
        // their walks wait for memory more than they issue (+5.8 %; the 3 k-point shape loses 3 % to the waves' uneven shares and stays with two).
        struct KSet { size_t (*shared_bytes)(int, int, int, int, int); int (*min_tile)(int, int, int); int (*tile_granule)(); int (*block_max)();
                      hipError_t (*launch)(int, int, int, int, int, int, int, hipStream_t, const PairDesc*, int, int, unsigned, unsigned long long*, const DevParams&, const unsigned*, unsigned*, const float* const*,
                                          int); };
        static const KSet KS2 = {align_shared_bytes, align_min_tile, align_tile_granule, align_block_max, launch_align};
        static const KSet KS3 = {cvohip_w3::align_shared_bytes, cvohip_w3::align_min_tile, cvohip_w3::align_tile_granule, cvohip_w3::align_block_max, cvohip_w3::launch_align};
        // a launch in an arithmetic mode (cvo_set_arith_mode / cvo_batch_set_arith_mode) runs the builds that have the modes, planned by their own LDS figures
        static const KSet KSE2 = {cvohip_e337::align_shared_bytes, cvohip_e337::align_min_tile, cvohip_e337::align_tile_granule, cvohip_e337::align_block_max, cvohip_e337::launch_align};
        static const KSet KSE3 = {cvohip_e337_w3::align_shared_bytes, cvohip_e337_w3::align_min_tile, cvohip_e337_w3::align_tile_granule, cvohip_e337_w3::align_block_max,
                                  cvohip_e337_w3::launch_align};
        const int arith_l = arith;                                   // (taken once: the launch keeps the mode it was queued with)
        const KSet& K2 = arith_l ? KSE2 : KS2; const KSet& K3 = arith_l ? KSE3 : KS3;
        struct Plan { int y_mode = 0, tile = 0, tab_cols = 0, block = 0; bool err = false; };
        const int rows_per_w = ((((std::max(nf_max, 1) + 127) / 128) + G - 1) / G) * 128;   // rows are dealt to the workgroups in blocks of 128 (ROW_DEAL)
        const int rows_cap = round_up(std::max(rows_per_w, 1), 128) + 64;
        auto plan = [&](const KSet& K) -> Plan {
        Plan pl;
        const int tgran = K.tile_granule();
        // LDS budget of one workgroup.  The transformed moving cloud is kept resident if at all possible: as float4 {y, g0}
        // (mode 1) beside a cull tile that holds the whole cloud; else as three float planes (mode 2, 12 B/point) beside a
        // tile just large enough to keep the fixed points in slot order; else it stays in HBM/L2 (mode 0).
        const size_t lds_cap = (size_t)(160 / per_cu - 4) * 1024;
        const int tile_full = std::min(round_up(std::max(nm_max, tgran), tgran), 4096);
        const int tile_rows = round_up(std::max(round_up(std::max(rows_per_w, 1), 64), 512), tgran);   // >= the slots: x_i by slot fits the idle tile
        const bool allow_lds = !std::getenv("CVO_HIP_NO_YLDS");
        int& y_mode = pl.y_mode; int& tile = pl.tile; y_mode = 0; tile = tile_request > 0 ? round_up(tile_request, tgran) : tile_full;
        if (const char* e = std::getenv("CVO_HIP_Y_MODE")) {                                // test knob: force a layout (must fit)
            y_mode = std::max(0, std::min(2, std::atoi(e)));
            if (tile_request <= 0) { tile = y_mode == 1 ? tile_full : std::min(tile_full, std::max(tile_rows, 512)); while (tile > tgran && K.shared_bytes(tile, rows_cap, y_mode, nm_pad, 0) > lds_cap) tile -= tgran; }
            tile = std::max(tile, K.min_tile(rows_cap, y_mode, nm_pad));
            if (K.shared_bytes(tile, rows_cap, y_mode, nm_pad, 0) > lds_cap) { pl.err = true; return pl; }
        } else if (tile_request > 0) {
            if (allow_lds && K.shared_bytes(tile, rows_cap, 1, nm_pad, 0) <= lds_cap) y_mode = 1;
            else if (allow_lds && K.shared_bytes(std::max(tile, K.min_tile(rows_cap, 2, nm_pad)), rows_cap, 2, nm_pad, 0) <= lds_cap) { y_mode = 2; tile = std::max(tile, K.min_tile(rows_cap, 2, nm_pad)); }
            else while (tile > tgran && K.shared_bytes(tile, rows_cap, 0, 0, 0) > lds_cap) tile -= tgran;
        } else {
            int t1 = tile_full; while (t1 > 512 && K.shared_bytes(t1, rows_cap, 1, nm_pad, 0) > lds_cap) t1 -= tgran;
            // plane layout: the tile only holds the fixed points by slot (and the rebuild scratch during a rebuild); it is not used for columns
            const int t2min = K.min_tile(rows_cap, 2, nm_pad);
            int t2 = std::max(std::min(tile_full, tile_rows), t2min); while (t2 > t2min && K.shared_bytes(t2, rows_cap, 2, nm_pad, 0) > lds_cap) t2 -= tgran;
            if (allow_lds && K.shared_bytes(t1, rows_cap, 1, nm_pad, 0) <= lds_cap) { y_mode = 1; tile = t1; }
            else if (allow_lds && K.shared_bytes(t2, rows_cap, 2, nm_pad, 0) <= lds_cap) { y_mode = 2; tile = t2; }
            else { tile = std::min(tile_full, 2048); while (tile > tgran && K.shared_bytes(tile, rows_cap, 0, 0, 0) > lds_cap) tile -= tgran; }
        }
        // line-search table (cvo_kernels.hip, phase L): 16 bytes per moving point behind the resident cloud, when that fits
        int& tab_cols = pl.tab_cols; tab_cols = 0;
        if (!std::getenv("CVO_HIP_NO_TABLE") && y_mode != 0 && K.shared_bytes(tile, rows_cap, y_mode, nm_pad, nm_pad) <= (size_t)(160 / per_cu) * 1024 - 512) tab_cols = nm_pad;
        const int bmax = K.block_max();
        int& block = pl.block; block = rows_per_w > bmax / 2 ? bmax : std::max(64, round_up(rows_per_w, 64));
        if (per_cu > 1) block = std::min(block, 256);
        if (block_request > 0) block = std::max(64, std::min(bmax, round_up(block_request, 64)));

        return pl;
        };
        const KSet* K = &K2;
        Plan pl = plan(K2);
        if (pl.err) return fail(CVO_ERR_INVALID, "CVO_HIP_Y_MODE: the requested LDS layout does not fit");
        if ((pl.y_mode == 2 || (wide_all && pl.y_mode == 1)) && wide_waves && per_cu == 1) {
            const Plan p3 = plan(K3);
            if (!p3.err && p3.y_mode == pl.y_mode) { pl = p3; K = &K3; }
        }
        const int y_mode = pl.y_mode, tile = pl.tile, tab_cols = pl.tab_cols, block = pl.block, rows_per = rows_per_w;

        int rc;
        if ((rc = d_descs.ensure(sizeof(PairDesc) * n))) return rc;
        if ((rc = h_descs.ensure(sizeof(PairDesc) * n))) return rc;
        if ((rc = d_states.ensure(sizeof(PairState) * (size_t)std::max(n, state_slots)))) return rc;
        if ((rc = d_records.grow_keep(sizeof(float) * CVO_RESULT_FLOATS * (size_t)std::max(n, rec_hint), 0, s))) return rc;
        if (n > pad_from) pad_from = pad_to = 0;                     // this launch writes over (some of) the padding records
        if ((rc = h_states.ensure(sizeof(PairState) * n))) return rc;
        if ((rc = h_states_in.ensure(sizeof(PairState) * n))) return rc;
        if (2 * (long long)P.max_iter + 8 >= 65536) return fail(CVO_ERR_INVALID, "max_iter must be below 32764");
        if ((rc = d_ybuf.ensure(sizeof(float4) * (size_t)slots * G * nm_pad))) return rc;   // work buffers: per pair SLOT of the launch
        // Adoption (a pair can grow to four workgroups while it runs): only for one workgroup and one slot per pair with the cloud resident
        // in LDS.  Every member keeps its lists and records in a region of its own, sized for the rows it owns when it joins (make_ctx:
        // 1 + 1/2 + 1/3 + 1/4 of the rows, each rounded up to blocks of 128), and the exchange area has room for four members
        // (cvo_kernels.hip: ADOPT_GMAX).
        AdoptCounters* const qc = adopt_counters(device);                   // what is queued on the device: every launch counts (null: the counters could not be made)
        AdoptCounters* const ac = (adopt && G == 1 && slots == n && y_mode != 0) ? qc : nullptr;
        const int gmax = align_adopt_gmax();                                 // the kernel's limit (ADOPT_GMAX)
        const int Gx = ac ? gmax : G;                                        // members a pair's exchange area has room for
        size_t member_rows = 0;                                              // rows of all member regions of a slot under adoption
        if (ac) { const int nbk = (std::max(nf_max, 1) + 127) / 128; for (int q = 1; q <= gmax; ++q) member_rows += (size_t)((nbk + q - 1) / q) * 128; }
        const size_t plane = ac ? member_rows * capf : (size_t)G * rows_per * capf;   // workgroup g's nonzero records start at g * rows_per * capf
        const int rows_pad = round_up(std::max(rows_per, 1), 128);          // the cull walks pairs of 64-row blocks
        int capn = 64; while (capn < nm_max / 3 && capn < 4096) capn *= 2;   // longest list a row may have: 1024 at 3 k points, 4096 at 10 k
        if (const char* e = std::getenv("CVO_HIP_ROW_CAP")) capn = std::max(1, std::atoi(e));
        capn = std::max(8, round_up(capn, 4));                               // the candidate phase reads entries four at a time, one step ahead
        const size_t tplane = ac ? member_rows * capn : (size_t)G * capn * rows_pad;
        if ((rc = d_jT.ensure(sizeof(uint16_t) * (size_t)slots * tplane))) return rc;
        if ((rc = d_ent.ensure(sizeof(uint2) * (size_t)slots * tplane))) return rc;
        if ((rc = d_surv.ensure(sizeof(uint2) * (size_t)slots * plane))) return rc;
        const size_t xch_bytes = sizeof(unsigned long long) * (size_t)n * 2 * Gx * XCH_WORDS;
        if ((rc = d_xch.ensure(xch_bytes))) return rc;
        if (want_trace) {
            if ((rc = d_trace.ensure(sizeof(TraceRow) * (size_t)std::max(1, trace_cap)))) return rc;
            if ((rc = d_tracelen.ensure(sizeof(int) * 4))) return rc;
            HIP_TRY(hipMemsetAsync(d_tracelen.p, 0, sizeof(int) * 4, s));
        }
        // the tracker's score block in the kernel's tail: the clouds' tables of cached self inner products live behind their group boxes
        bool tails = tail_scores && !want_trace;
        for (int i = 0; i < n && tails; ++i) tails = pairs[i].fixed && pairs[i].moving && pairs[i].fixed->n > 0 && pairs[i].moving->n > 0;
        // clouds handed over since the last launch: packed by this launch's workgroups (one per pair, nothing that needs the clouds before the
        // kernel runs), else by the pack kernel now
        const float** rawtab = nullptr;
        if (!pending.empty()) {
            if (inkernel_pack && G == 1 && !tails) {
                if (launched && last_stream) HIP_TRY(hipStreamSynchronize(last_stream));   // an earlier launch of this engine may still read the table
                if ((rc = h_rawtab.ensure(sizeof(const float*) * 4 * (size_t)n))) return rc;
                rawtab = static_cast<const float**>(h_rawtab.p);
                // (the clouds' raw pointers are host addresses in the ring; with the mirror the kernel gets the same offsets in the device copy)
                const bool mir = ring_mirror && d_ring.p && d_ring.bytes >= h_stage.bytes && ev_ring;
                const ptrdiff_t shift = mir ? (static_cast<const unsigned char*>(d_ring.p) - static_cast<const unsigned char*>(h_stage.p)) : 0;
                auto dev = [&](const float* r) -> const float* { return r ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(r) + shift) : nullptr; };
                for (int i = 0; i < n; ++i) {                        // {positions, features (null: right behind the positions)} x {fixed, moving}
                    const Cloud* cf = pairs[i].fixed; const Cloud* cm = pairs[i].moving;
                    rawtab[4 * i] = dev(cf ? cf->raw : nullptr); rawtab[4 * i + 1] = (cf && cf->raw) ? cf->raw_feat : nullptr;
                    rawtab[4 * i + 2] = dev(cm ? cm->raw : nullptr); rawtab[4 * i + 3] = (cm && cm->raw) ? cm->raw_feat : nullptr;
                }
                if (mir && s != stream) HIP_TRY(hipStreamWaitEvent(s, ev_ring, 0));
            } else if ((rc = flush_pending(s))) return rc;
        }
        if (tails) {
            if ((rc = h_tail.ensure(sizeof(double) * (size_t)n * 5 * 24))) return rc;
            for (int i = 0; i < n; ++i) { if ((rc = ensure_boxes(*pairs[i].fixed, s))) return rc; if ((rc = ensure_boxes(*pairs[i].moving, s))) return rc; }
        }
        std::vector<PairDesc> hdv(n);
        std::memset(hdv.data(), 0, sizeof(PairDesc) * n);            // padding bytes take part in the comparison below
        PairDesc* hd = hdv.data();
        // Which pair a position of the launch (a slot; a pull from the pair queue) works on.  A pair's time is its cost per iteration -- which
        // follows the number of neighbours, i.e. the density of its clouds: mean 1/z^2 explains 0.9 of it on the bench's pairs, the iteration
        // count next to nothing -- so the pairs are ranked by that (Cloud::cost_hint, a sample of the points taken at the hand-over), and
        //  * a launch with a slot per pair gives the positions b, b + 8, b + 16, ... -- workgroups that share an XCD: block p of a launch runs on XCD
        //    (h + p) mod 8, h fixed per stream and different from stream to stream (scripts/micro/xcc_map.hip) -- pairs of SIMILAR density: the c-th
        //    eighth of the ranking goes to the positions = c (mod 8).  With eight streams the launches then form a Latin square over the XCDs: every
        //    XCD hosts every density class, each from another stream, eight pairs of one class at a time -- equal work per XCD, and the eight CUs a
        //    class leaves come free together for the next launch's eight blocks on that XCD.  Measured: +5.3 ... +6.4 % over index order on four sets
        //    of 64 pairs, +11 % with 512 different pairs in flight; evenly mixed orders (densest first, eight heavy / eight light) lose 2 ... 13 %,
        //    2 / 4 / 16 / 32 classes instead of 8 lose 4 / 2 / 13 / 22 %, and launches that disagree on the classes' positions lose 35 %
        //    (profiles/r03_pair_order_*.txt, r03_distinct_sets_ab.txt, r03_class_count_sweep.txt, r03_class_shift_across_handles.txt);
        //  * a launch with fewer slots than pairs hands them out densest first: the long pairs start first and the launch's last ones are
        //    short (+5 ... 13 % on the config-5 shape, 64 pairs on 10 slots).
        // Results stay indexed by pair.  CVO_HIP_ORDER_PAIRS: 0 index order, 1 this rule (default); 2 ... experiment orders (below).
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        if (order_pairs && n > 1) {
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                const float ca = (pairs[a].fixed ? pairs[a].fixed->cost_hint : 0.f) + (pairs[a].moving ? pairs[a].moving->cost_hint : 0.f);
                const float cb = (pairs[b].fixed ? pairs[b].fixed->cost_hint : 0.f) + (pairs[b].moving ? pairs[b].moving->cost_hint : 0.f);
                return ca > cb; });
            const bool queue_launch = slots < n;
            // The XCD-class rule presumes that the positions = c (mod 8) of the launch are the blocks = c (mod 8): one workgroup per pair, or a pair's workgroups
            // co-located on the blocks of one class (DevParams::colocate with the slots a multiple of eight).  A cooperative launch with consecutive blocks per pair
            // spreads every pair over several XCDs whatever its position: densest first there, like the queue launches.  The density ranking itself (Cloud::cost_hint,
            // the mean of 1/z^2 over a sample of the points) presumes clouds in the camera frame with +z the viewing direction, as pcd_generator makes them
            // (pcd_generator.cpp:471-476); clouds in another frame get an arbitrary but harmless ranking -- CVO_HIP_ORDER_PAIRS=0 keeps index order.
            const bool class_is_xcd = G == 1 || (P.colocate && (slots & 7) == 0);
            const int mode = order_mode == 1 ? ((queue_launch || !class_is_xcd) ? 2 : 5) : order_mode;      // 2 densest first, 5 eighths of the ranking per XCD class
            if (mode == 3) std::reverse(order.begin(), order.end());                      // lightest first
            if (mode == 4) { std::vector<int> o2; for (int i = 0, j = n - 1; i <= j; ++i, --j) { o2.push_back(order[i]); if (i != j) o2.push_back(order[j]); } order = o2; }   // heavy, light, heavy, ...
            if (mode == 5 || mode == 10 || mode == 11) {                                   // position p <- chunk p % 8 of the ranking, its (p / 8)-th pair
                std::vector<int> first(9, 0), o2(n);
                for (int c = 0; c < 8; ++c) first[c + 1] = first[c] + n / 8 + ((mode == 11 ? 7 - c : c) < n % 8 ? 1 : 0);   // a chunk has as many pairs as its class has positions
                for (int p = 0; p < n; ++p) {
                    const int c = mode == 11 ? 7 - p % 8 : p % 8, len = first[c + 1] - first[c];
                    const int k = p / 8;                                                  // experiment orders: 10 lightest of the chunk first, 11 chunks in reverse
                    o2[p] = order[first[c] + (mode == 10 ? len - 1 - k : k)];
                }
                order = o2;
            }
            if (mode >= 20 && mode < 100) {                                                // experiment: K = mode - 20 classes instead of 8 (position p <- chunk p % K, its (p / K)-th pair)
                const int Kc = std::max(1, std::min(n, mode - 20));
                std::vector<int> first(Kc + 1, 0), o2(n);
                for (int c = 0; c < Kc; ++c) first[c + 1] = first[c] + n / Kc + (c < n % Kc ? 1 : 0);
                for (int p = 0; p < n; ++p) o2[p] = order[first[p % Kc] + p / Kc];
                order = o2;
            }
            if (mode == 6) { std::vector<int> o2; const int nb8 = (n + 7) / 8; for (int i = 0, j = nb8 - 1; i <= j; ++i, --j) { for (int q = 8 * i; q < std::min(n, 8 * i + 8); ++q) o2.push_back(order[q]); if (i != j) for (int q = 8 * j; q < std::min(n, 8 * j + 8); ++q) o2.push_back(order[q]); } order = o2; }   // eight heavy, eight light, ...
            if (mode >= 7 && mode < 10) { unsigned st = 12345u * (unsigned)mode; for (int i = n - 1; i > 0; --i) { st = st * 1664525u + 1013904223u; std::swap(order[i], order[(st >> 8) % (unsigned)(i + 1)]); } }   // shuffles
        }
        for (int i = 0; i < n; ++i) {
            PairDesc& D = hd[i];
            D.fixed = pairs[i].fixed ? pairs[i].fixed->rec() : nullptr;
            D.moving = pairs[i].moving ? pairs[i].moving->rec() : nullptr;
            D.nf = pairs[i].fixed ? pairs[i].fixed->n : 0;
            D.nm = pairs[i].moving ? pairs[i].moving->n : 0;
            D.nf_pad = nf_pad; D.rows_pad = rows_pad; D.capf = capf; D.nm_pad = nm_pad;
            D.ybuf = static_cast<float4*>(d_ybuf.p);
            D.ws_y_stride = (long long)G * nm_pad; D.ws_list_stride = (long long)tplane; D.ws_surv_stride = (long long)plane;
            D.capn = capn;
            D.jT = static_cast<uint16_t*>(d_jT.p);
            D.ent = static_cast<uint2*>(d_ent.p);
            D.surv = static_cast<uint2*>(d_surv.p);
            D.xch = static_cast<unsigned long long*>(d_xch.p) + (size_t)i * 2 * Gx * XCH_WORDS;
            D.state = static_cast<PairState*>(d_states.p) + (state_index ? state_index[i] : i);
            D.state_in = (upload_each ? upload_each[i] != 0 : upload_states) ? static_cast<const PairState*>(h_states_in.p) + i : D.state;
            D.state_host = static_cast<PairState*>(h_states.p) + i;
            D.trace = (want_trace && i == 0) ? static_cast<TraceRow*>(d_trace.p) : nullptr;
            D.trace_cap = want_trace ? trace_cap : 0;
            D.trace_len = want_trace ? static_cast<int*>(d_tracelen.p) : nullptr;
            D.member_regions = ac ? 1 : 0;
            D.run_pair = order[i];
            D.record = static_cast<float*>(d_records.p) + (size_t)i * CVO_RESULT_FLOATS;
            if (tails) {
                D.score_out = static_cast<double*>(h_tail.p) + (size_t)i * 5 * 24;
                D.self_fixed = score_self_cache(static_cast<float*>(pairs[i].fixed->boxes.p), pairs[i].fixed->n);
                D.self_moving = score_self_cache(static_cast<float*>(pairs[i].moving->boxes.p), pairs[i].moving->n);
            }
        }
        // Steady state = no copy-engine work at all: copies queued on different streams share the DMA engines and a copy behind
        // another stream's running kernel would serialise the launches.  Descriptors go up only when they changed, start states
        // are read by the kernel from pinned host memory, final states are written by it to pinned host memory, and the
        // exchange area is cleared only when it is new (tags carry the launch number).
        if (descs_uploaded.size() != sizeof(PairDesc) * n || std::memcmp(descs_uploaded.data(), hd, sizeof(PairDesc) * n) != 0) {
            if (!queue_behind) HIP_TRY(hipStreamSynchronize(s));      // an earlier launch on this stream may still read d_descs / h_descs
            else if (launched) HIP_TRY(hipEventSynchronize(ev1));
            std::memcpy(h_descs.p, hd, sizeof(PairDesc) * n);
            HIP_TRY(hipMemcpyAsync(d_descs.p, h_descs.p, sizeof(PairDesc) * n, hipMemcpyHostToDevice, s));
            descs_uploaded.assign(reinterpret_cast<const unsigned char*>(hd), reinterpret_cast<const unsigned char*>(hd) + sizeof(PairDesc) * n);
        }
        bool any_upload = upload_states && !upload_each;
        for (int i = 0; upload_each && i < n && !any_upload; ++i) any_upload = upload_each[i] != 0;
        if (any_upload) {
            if (launched) HIP_TRY(hipStreamSynchronize(last_stream));  // a queued launch of this engine may not have read its start states yet
            std::memcpy(h_states_in.p, states_in, sizeof(PairState) * n);
        }
        launch_seq = (launch_seq + 1) & 0xFFFFu;
        {   // pair queue of launches with fewer slots than pairs: head word + one mailbox per slot; tags carry the launch number
            const size_t qbytes = sizeof(unsigned long long) * (size_t)(1 + 2 * num_cus * per_cu);   // head, a mailbox / adoption word per slot, a control word per slot
            const bool fresh = d_queue.bytes < qbytes;
            if ((rc = d_queue.ensure(qbytes))) return rc;
            if (fresh || launch_seq == 0) HIP_TRY(hipMemsetAsync(d_queue.p, 0, d_queue.bytes, s));
        }
        if (Gx > 1 && (xch_zeroed_bytes != d_xch.bytes || launch_seq == 0)) {
            HIP_TRY(hipMemsetAsync(d_xch.p, 0, d_xch.bytes, s));
            xch_zeroed_bytes = d_xch.bytes;
        }
        for (hipEvent_t ev : run_after) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        HIP_TRY(hipEventRecord(ev0, s));
        hipError_t e;
        DevParams Pl = P;
        // The list margin: a moving point may travel skin * r + skin_alpha * (its distance from the camera) before the lists are stale (DevParams::skin_alpha).  Round 3 had one
        // margin for all rows (0.35 r / 0.30 r by layout); with the depth-proportional part the constant part shrinks to what a translation needs, the lists of the near (dense) rows
        // get shorter and the pairs cull 2.0-2.3 times instead of 3.3-3.8: +10 % at 3 k points, +6 % at 9 k (profiles/r04_list_margin_sweep.txt; other motion mixes: r04_list_margin_motion.txt)
        if (skin_auto && alpha_auto) { Pl.skin = y_mode == 1 ? 0.05f : 0.15f; Pl.skin_alpha = y_mode == 1 ? 0.0125f : 0.01f; if (!gamma_set) Pl.alpha_gamma = y_mode == 1 ? 1.0f : 0.f; }
        else if (skin_auto) Pl.skin = y_mode == 1 ? 0.35f : 0.30f;   // CVO_HIP_SKIN_ALPHA given alone: the constant part as round 3 had it
        // Wider FIRST lists for the pairs of a BATCH on four or more cooperating workgroups each (a handful of loop-closure candidates, keyframe_graph.cpp:693-717: few rows per
        // workgroup, a cull costs what it always did, and the frames are far apart): 1.75 x the margin, most pairs then cull once instead of twice -- 10 candidates 2.53 -> 2.35 ms, one
        // of the bench's pairs alone -2.2 %.  Not for single handles: a tracker's consecutive frames cull once either way and the wider lists ADD 5 % to their alignments
        // (profiles/r04_single_pair_phases.txt).  CVO_HIP_FIRST_SCALE sets it for every launch.
        if (coop_first_scale > 0.f && !first_scale_set && G >= 4 && y_mode == 1) Pl.first_scale = coop_first_scale;
        Pl.adopt_on = ac ? ADOPT_ON_HELP : 0;
        int grid_l = grid, concurrent = 1;
        if (qc) {                                                     // count the workgroups as submitted, then submit them: in that order, under one lock per process
            std::lock_guard<std::mutex> lk(adopt_submit_mutex());
            bool deferred = false;
            launch_share(&concurrent, &deferred);
            // An adoption launch whose share of the device holds more workgroups than it has pairs brings helpers along: workgroups n ... grid - 1 join
            // pairs from their first iterations (cvo_align_kernel), up to ADOPT_GMAX workgroups per pair.  Otherwise the launch is what it always was.
            const int share = std::min(num_cus * per_cu / concurrent, max_wgs > 0 ? max_wgs : num_cus * per_cu);
            if (ac && share > n) grid_l = std::min(share, gmax * n);
            if (deferred) Pl.adopt_on |= ADOPT_ON_DEFERRED;
            if (!deferred) *qc->submitted_host += (unsigned)grid_l;
            e = K->launch(grid_l, block, tile, rows_cap, y_mode, nm_pad, tab_cols, s, static_cast<const PairDesc*>(d_descs.p), n, G, launch_seq << 16, static_cast<unsigned long long*>(d_queue.p), Pl,
                             qc->submitted_dev, qc->started_dev, rawtab, arith_l);
            if (e != hipSuccess) resync_adopt_counters(qc);
            else e = hipEventRecord(ev1, s);                          // under the lock: launch_share of other engines queries it
            launched = launched || e == hipSuccess;
        } else {
            e = K->launch(grid, block, tile, rows_cap, y_mode, nm_pad, tab_cols, s, static_cast<const PairDesc*>(d_descs.p), n, G, launch_seq << 16, static_cast<unsigned long long*>(d_queue.p), Pl, nullptr, nullptr, rawtab, arith_l);
            if (e == hipSuccess) e = hipEventRecord(ev1, s);
        }
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("align kernel launch: ") + hipGetErrorString(e));
        last_grid = grid_l; last_helpers = grid_l - grid; last_concurrent = concurrent;
        launched = true;
        last_stream = s;
        last_tail = tails;
        if (rawtab) {                                                 // those clouds are the kernel's now; the ring has to stay as it is until the launch is over
            for (int i = 0; i < n; ++i) { if (pairs[i].fixed) { pairs[i].fixed->raw = nullptr; pairs[i].fixed->raw_feat = nullptr; } if (pairs[i].moving) { pairs[i].moving->raw = nullptr; pairs[i].moving->raw_feat = nullptr; } }
            pending.erase(std::remove_if(pending.begin(), pending.end(), [](Cloud* c) { return c->raw == nullptr; }), pending.end());
            add_ring_reader(s);
        }
        return CVO_OK;
    }
    hipStream_t last_stream = nullptr;

    // The block of n_block records this engine contributes to a cross-GPU gather, complete on *s_out in stream order: records
    // [0, n_valid) are the last launch's (written by the align kernel), [n_valid, n_block) stand for no pair and carry CVO_ERR_PADDING --
    // blocks differ by one pair between ranks when the pairs do not divide evenly (cvo_shard_range), the collective needs equal counts.
    // launch_status != CVO_OK: this rank's launch could not be made; all n_block records carry that status, so the rank still takes part
    // in the collective and every rank learns of the failure instead of waiting for it forever.
    int padded_records(int n_valid, int n_block, int launch_status, int last_n, hipStream_t* s_out, float** send) {
        HIP_TRY(hipSetDevice(device));
        if (n_block <= 0 || n_valid < 0 || n_valid > n_block) return fail(CVO_ERR_INVALID, "gather: need 0 <= n_valid <= n_block, n_block > 0");
        if (launch_status == CVO_OK && n_valid > 0 && (!launched || n_valid > last_n)) return fail(CVO_ERR_INVALID, "gather: more records than the last launch aligned");
        hipStream_t s = launched ? last_stream : stream;
        const int keep = launch_status == CVO_OK ? n_valid : 0;
        int rc = d_records.grow_keep(sizeof(float) * CVO_RESULT_FLOATS * (size_t)n_block, sizeof(float) * CVO_RESULT_FLOATS * (size_t)keep, s); if (rc) return rc;
        const int from = keep, status = launch_status == CVO_OK ? CVO_ERR_PADDING : launch_status;
        if (from < n_block && !(pad_from == from && pad_to >= n_block && pad_status == status)) {
            const hipError_t e = launch_fill_records(static_cast<float*>(d_records.p), from, n_block, status, s);
            if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("record fill kernel launch: ") + hipGetErrorString(e));
            pad_from = from; pad_to = n_block; pad_status = status;
        }
        *s_out = s; *send = static_cast<float*>(d_records.p);
        return CVO_OK;
    }

    int wait() {
        HIP_TRY(hipSetDevice(device));
        if (!launched) return fail(CVO_ERR_INVALID, "no launch to wait for");
        const hipError_t es = hipStreamSynchronize(last_stream);
        release_slots();                                             // the launch has left the device, whatever it returned
        if (es != hipSuccess) return fail(CVO_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
        HIP_TRY(hipEventElapsedTime(&last_ms, ev0, ev1));
        return CVO_OK;
    }
    // the align kernel has finished (its states are in h_states, which it writes itself); work queued behind it on the stream may still run
    int wait_align_only() {
        HIP_TRY(hipSetDevice(device));
        if (!launched) return fail(CVO_ERR_INVALID, "no launch to wait for");
        const hipError_t es = hipEventSynchronize(ev1);
        release_slots();
        if (es != hipSuccess) return fail(CVO_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(es));
        HIP_TRY(hipEventElapsedTime(&last_ms, ev0, ev1));
        return CVO_OK;
    }
    const PairState* results() const { return static_cast<const PairState*>(h_states.p); }

    // function_inner_product / se3_Hessian: out[0]=sum_A, out[1]=count, out[2..22]=Hessian terms
    // A score block: any number of function_inner_product / se3_Hessian evaluations in one launch.
    // out[r][0] = sum_A, out[r][1] = pair count, out[r][2..22] = Hessian terms.
    struct ScoreReq {
        const Cloud* a; const float* tran; const Cloud* b; bool hessian; float ell;
        int from = -1;                    // >= 0: ell comes from pair `from`'s device-resident state (the align() result, Q1) ...
        bool tran_from_state = false;     // ... and so does the transform applied to cloud a
    };
    DevBuf d_scoredescs; PinBuf h_scoredescs;
    bool self_cache_on = true;        // CVO_HIP_SELF_CACHE=0: every fip(cloud, cloud) is swept again (tests compare the two)
    std::vector<unsigned char> scoredescs_uploaded;
    hipStream_t score_stream = nullptr; int score_pending = 0;
    size_t stage_used = 0;            // bytes of the pinned staging ring handed to copies that may still be in flight
    bool uploads_pending = false;     // clouds were written on `stream`: a launch on another stream waits for them once
    int settle_uploads(hipStream_t s) {
        if (uploads_pending && s != stream) HIP_TRY(hipStreamSynchronize(stream));
        uploads_pending = false;
        return CVO_OK;
    }
    int ensure_boxes(const Cloud& c, hipStream_t s) {
        if (!c.boxes_valid) {
            int rc = c.boxes.ensure(score_box_bytes(c.n)); if (rc) return rc;
            hipError_t e = launch_cloud_boxes(c.rec(), c.n, static_cast<float*>(c.boxes.p), s);
            if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("cloud box kernel launch: ") + hipGetErrorString(e));
            c.boxes_valid = true; c.boxes_stream = s;
        } else if (c.boxes_stream != s) {
            HIP_TRY(hipStreamSynchronize(c.boxes_stream));           // made on another stream of this engine: complete before use here
            c.boxes_stream = s;
        }
        return CVO_OK;
    }
    // A counted sweep launch.  The workgroups of a score, support, match, hypothesis or pose-model sweep are queued work that the helpers of align
    // launches in flight hold back for (AdoptCounters), and this is the one copy of what the host owes them: `wgs` joins `submitted` before the
    // launch, leaves it again when the sweep was never handed to the runtime (nothing of it will start), and a launch call that reports an error
    // after that re-synchronises the counters.  launch(wgs_started, sweep_submitted) -> hipError_t; both null on a device without counters.
    template <class Launch> hipError_t counted_sweep(unsigned wgs, Launch&& launch) {
        AdoptCounters* const qc = adopt_counters(device);
        if (!qc) return launch(static_cast<unsigned*>(nullptr), static_cast<bool*>(nullptr));
        std::lock_guard<std::mutex> lk(adopt_submit_mutex());
        *qc->submitted_host += wgs;
        bool sweep_submitted = false;
        const hipError_t e = launch(qc->started_dev, &sweep_submitted);
        if (!sweep_submitted) *qc->submitted_host -= wgs;
        else if (e != hipSuccess) resync_adopt_counters(qc);
        return e;
    }
    // Queue the launch on stream s; the sums land in pinned memory when s has drained (score_collect).
    int score_enqueue(const ScoreReq* rq, int n, hipStream_t s) {
        HIP_TRY(hipSetDevice(device));
        if (n <= 0) return fail(CVO_ERR_INVALID, "bad score request count");
        { int rcs = flush_pending(s); if (rcs) return rcs; }
        { int rcs = settle_uploads(s); if (rcs) return rcs; }
        std::vector<ScoreDesc> descs(n);
        int row_blocks = 1;
        for (int r = 0; r < n; ++r) {
            if (!rq[r].a || !rq[r].b || rq[r].a->n <= 0 || rq[r].b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "empty cloud");
            ScoreDesc& D = descs[r];
            std::memset(&D, 0, sizeof(D));
            int rcb = ensure_boxes(*rq[r].b, s); if (rcb) return rcb;
            D.a = rq[r].a->rec(); D.b = rq[r].b->rec(); D.na = rq[r].a->n; D.nb = rq[r].b->n; D.ell = rq[r].ell;
            D.bbox = static_cast<const float*>(rq[r].b->boxes.p); D.nbox = score_groups(D.nb);
            D.want_hessian = rq[r].hessian ? 1 : 0; D.out = nullptr;
            // fip(cloud, cloud), untransformed: a function of the cloud and ell alone (cvo.cpp:496-497), kept with the cloud
            if (self_cache_on && rq[r].a == rq[r].b && !rq[r].hessian && !rq[r].tran && !rq[r].tran_from_state)
                D.self_cache = score_self_cache(static_cast<float*>(rq[r].b->boxes.p), rq[r].b->n);
            // (a cloud that several pairs hold is asked about once per pair, each with its own ell: one request of a launch keeps the table, two workgroups never fill one entry)
            for (int q = 0; q < r && D.self_cache; ++q) if (descs[q].self_cache == D.self_cache) D.self_cache = nullptr;
            D.from = rq[r].from >= 0 ? static_cast<const PairState*>(d_states.p) + rq[r].from : nullptr;
            if (rq[r].tran_from_state && !D.from) return fail(CVO_ERR_INVALID, "score request: transform from a state that is not named");
            D.use_tran = rq[r].tran_from_state ? 2 : (rq[r].tran ? 1 : 0);
            for (int i = 0; i < 12; ++i) D.tran[i] = (rq[r].tran && !rq[r].tran_from_state) ? rq[r].tran[i] : 0.f;
            row_blocks = std::max(row_blocks, score_row_blocks(D.na));
        }
        const int nout = score_nout();
        const int chunks = std::max(1, std::min(16, 4 * num_cus / std::max(1, row_blocks * n)));   // ~4 workgroups (waves) per CU
        int rc;
        if ((rc = d_partials.ensure(sizeof(double) * (size_t)n * row_blocks * chunks * nout))) return rc;
        if ((rc = h_partials.ensure(sizeof(double) * (size_t)std::max(n, SCORE_MAXREQ) * nout))) return rc;
        ScoreBatch B; std::memset(&B, 0, sizeof(B));
        const ScoreDesc* more = nullptr;
        if (n <= SCORE_MAXREQ) { B.n = n; for (int r = 0; r < n; ++r) B.d[r] = descs[r]; }
        else {
            // like the align descriptors: uploaded only when they changed, so a steady stream of score blocks over the same pairs
            // (transforms taken from the device-resident states) queues no copy
            const size_t bytes = sizeof(ScoreDesc) * (size_t)n;
            if (scoredescs_uploaded.size() != bytes || std::memcmp(scoredescs_uploaded.data(), descs.data(), bytes) != 0) {
                if ((rc = d_scoredescs.ensure(bytes))) return rc;
                if ((rc = h_scoredescs.ensure(bytes))) return rc;
                HIP_TRY(hipStreamSynchronize(s));
                std::memcpy(h_scoredescs.p, descs.data(), bytes);
                HIP_TRY(hipMemcpyAsync(d_scoredescs.p, h_scoredescs.p, bytes, hipMemcpyHostToDevice, s));
                scoredescs_uploaded.assign(reinterpret_cast<const unsigned char*>(descs.data()), reinterpret_cast<const unsigned char*>(descs.data()) + bytes);
            }
            more = static_cast<const ScoreDesc*>(d_scoredescs.p);
        }
        const hipError_t e = counted_sweep((unsigned)row_blocks * (unsigned)chunks * (unsigned)n, [&](unsigned* wgs_started, bool* sweep_submitted) {
            return launch_score(B, more, n, row_blocks, chunks, P, static_cast<double*>(d_partials.p), static_cast<double*>(h_partials.p), s, wgs_started, sweep_submitted);
        });
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("score kernel launch: ") + hipGetErrorString(e));
        score_stream = s; score_pending = n;
        return CVO_OK;
    }
    int score_collect(int n, double (*out)[24]) {
        HIP_TRY(hipSetDevice(device));
        if (n <= 0 || n != score_pending) return fail(CVO_ERR_INVALID, "no queued score block of that size");
        HIP_TRY(hipStreamSynchronize(score_stream));
        const int nout = score_nout();
        const double* hp = static_cast<const double*>(h_partials.p);
        for (int r = 0; r < n; ++r) for (int q = 0; q < 24; ++q) out[r][q] = q < nout ? hp[(size_t)r * nout + q] : 0.0;
        score_pending = 0;
        return CVO_OK;
    }
    int score_many(const ScoreReq* rq, int n, double (*out)[24]) {
        int rc = score_enqueue(rq, n, stream); if (rc) return rc;
        return score_collect(n, out);
    }

    // ---- side calls: per-point support, point matches, pose hypotheses, pose models
    // What one kind of side call keeps from its enqueue to its collect.  Every kind has a record of its own (support_call, match_call, hyp_call,
    // pm_call): nothing in it is shared with another kind or with a score block, so a call of one kind may be in flight while another is queued.
    // One call of a kind at a time: begin() waits for the one before.
    struct SideCall {
        struct Copy { void* dst; size_t off, bytes; };
        const char* none_queued;                   // collect()'s error text when no call is queued
        hipEvent_t done = nullptr, in = nullptr;   // done: the call has left the device; in: where the caller's out_stream stood when the call was queued
        bool queued = false; hipStream_t stream = nullptr;
        DevBuf d_tab; PinBuf h_tab;                // the call's table: filled in h_tab, uploaded to d_tab
        DevBuf d_work;                             // moved planes and their boxes (support, matches); the sweep's partials (hypotheses, pose models)
        DevBuf d_out; PinBuf h_out;                // answers: the kernels write h_out themselves (hypotheses, pose models), or d_out, copied to h_out behind
        size_t out_bytes = 0; std::vector<Copy> copies;   // them (out_bytes > 0) and from there to the caller's host arrays by collect()
        int (Engine::*before_reuse)();             // non-null: begin() calls it before the last call's answers are given up (hypotheses: hyp_keep)
        explicit SideCall(const char* none_queued_text, int (Engine::*keep)() = nullptr) : none_queued(none_queued_text), before_reuse(keep) {}
        int wait() {
            if (queued) { HIP_TRY(hipEventSynchronize(done)); queued = false; }
            return CVO_OK;
        }
        // the last call's table, work buffer and answers are free; s is ready for the clouds; wait_align: an align launch on a caller's stream packs
        // clouds and writes states, so s waits for it
        int begin(Engine& E, hipStream_t s, bool wait_align) {
            if (!done) HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
            int rc;
            if ((before_reuse && (rc = (E.*before_reuse)())) || (rc = wait())) return rc;
            copies.clear(); out_bytes = 0;
            if ((rc = E.flush_pending(s)) || (rc = E.settle_uploads(s))) return rc;
            if (wait_align && E.launched && E.last_stream && E.last_stream != s) HIP_TRY(hipStreamWaitEvent(s, E.ev1, 0));
            return CVO_OK;
        }
        // whatever out_stream still does to the caller's device arrays comes before the call on s
        int order_after(hipStream_t out_stream, hipStream_t s) {
            if (!out_stream || out_stream == s) return CVO_OK;
            if (!in) HIP_TRY(hipEventCreateWithFlags(&in, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(in, out_stream));
            HIP_TRY(hipStreamWaitEvent(s, in, 0));
            return CVO_OK;
        }
        int upload(size_t tab_bytes, hipStream_t s) {
            HIP_TRY(hipMemcpyAsync(d_tab.p, h_tab.p, tab_bytes, hipMemcpyHostToDevice, s));
            return CVO_OK;
        }
        int finish(hipStream_t s) {
            if (out_bytes) HIP_TRY(hipMemcpyAsync(h_out.p, d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(done, s));
            queued = true; stream = s;
            return CVO_OK;
        }
        // waits for the call queued last; its host arrays are filled here
        int collect() {
            if (!queued) return fail(CVO_ERR_INVALID, none_queued);
            int rc = wait(); if (rc) return rc;
            for (const Copy& c : copies) std::memcpy(c.dst, static_cast<const unsigned char*>(h_out.p) + c.off, c.bytes);
            copies.clear();
            return CVO_OK;
        }
        // the device form's ordering with an out_stream: that stream waits for the call and the host does not (Engine::side_publish)
        int publish(hipStream_t out_stream) {
            if (out_stream != stream) HIP_TRY(hipStreamWaitEvent(out_stream, done, 0));
            return CVO_OK;
        }
        void release() {
            if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); done = nullptr; }   // (a device-form call may sit on a caller's stream)
            if (in) { (void)hipEventDestroy(in); in = nullptr; }
            queued = false;
            d_tab.release(); d_work.release(); d_out.release(); h_tab.release(); h_out.release();
        }
    };
    SideCall support_call{"no queued point support"}, match_call{"no queued point matches"}, hyp_call{"no queued hypothesis scores", &Engine::hyp_keep}, pm_call{"no queued pose models"};
    int side_collect(SideCall& C) { HIP_TRY(hipSetDevice(device)); return C.collect(); }
    // a call's end as its form asks: with an out_stream that stream waits, else the host does
    int side_publish(SideCall& C, hipStream_t out_stream) { return out_stream ? C.publish(out_stream) : side_collect(C); }

    // Per-point support (cvo_support_kernels.hip; include/cvo_hip.h: cvo_point_support) and point matches (cvo_match_kernels.hip; cvo_point_matches):
    // for every request the rows of a against the columns of b (dst.*_moving, a->n rows) and the roles swapped (dst.*_fixed, b->n rows); a direction
    // whose arrays are null is not computed.  ell and the transform as a ScoreReq names them.  to_host: the arrays are host memory, filled by
    // side_collect; else device memory the caller owns (checked by the entry point), written by the kernels themselves.
    template <class Dst> struct SideReq {
        const Cloud* a; const float* tran; const Cloud* b; float ell;
        int from; bool tran_from_state;
        Dst dst;
    };
    using SupportReq = SideReq<cvo_point_support_dst>;
    using MatchReq = SideReq<cvo_point_matches_dst>;
    static bool rows_moving(const cvo_point_support_dst& d) { return d.sum_moving != nullptr; }
    static bool rows_fixed(const cvo_point_support_dst& d) { return d.sum_fixed != nullptr; }
    static bool rows_moving(const cvo_point_matches_dst& d) { return d.best_moving != nullptr; }
    static bool rows_fixed(const cvo_point_matches_dst& d) { return d.best_fixed != nullptr; }
    // where a direction's outputs go: the caller's device memory as it is, or (to_host) a place in the call's d_out with its copy to the caller's array;
    // per-direction records (the matches' fit records) lie first, so that they stay 8-byte aligned, the row arrays behind them
    struct SideOut {
        SideCall& C; bool to_host; size_t head_at, rows_at;
        template <class T> T* put(T* dst, size_t& at, size_t bytes) {
            if (!to_host) return dst;
            C.copies.push_back(SideCall::Copy{dst, at, bytes});
            T* const p = reinterpret_cast<T*>(static_cast<unsigned char*>(C.d_out.p) + at); at += bytes; return p;
        }
        template <class T> T* rows(T* dst, size_t bytes) { return put(dst, rows_at, bytes); }
        template <class T> T* head(T* dst, size_t bytes) { return put(dst, head_at, bytes); }
    };
    // what a built call hands its launcher: the three parts of the device table (side calls of two directions) or the table itself (hypotheses, pose models)
    struct SidePlan {
        int n_moves = 0, n_move_max = 0, n_dirs = 0, row_blocks = 1; size_t tab_bytes = 0;
        const SupportMoveDesc* d_mv = nullptr; const BoxDesc* d_bx = nullptr; const void* d_descs = nullptr;
    };
    // Everything a support and a matches call have in common between begin() and the launch: what the call needs -- a moved {x, y, z, f0} plane and
    // its boxes per transformed cloud, the table (moves, boxes, one Desc per computed direction) and, to_host, a place per output (row_bytes a row,
    // head_bytes a direction) -- then the moves, the boxes and each direction's SweepSide, the roles swapped for the second one.
    // outputs(D, dst, swapped, rows, out) sets the kind's own output pointers of one direction.
    template <class Desc, class Dst, class Outputs>
    int build_sides(SideCall& C, const SideReq<Dst>* rq, int n, hipStream_t s, bool to_host, size_t row_bytes, size_t head_bytes, int (*row_blocks_of)(int),
                    Outputs&& outputs, SidePlan& pl) {
        size_t moved_bytes = 0, out_bytes = 0;
        for (int r = 0; r < n; ++r) {
            const int na = rq[r].a->n, nb = rq[r].b->n;
            if (rq[r].tran || rq[r].tran_from_state) { ++pl.n_moves; pl.n_move_max = std::max(pl.n_move_max, na); moved_bytes += sizeof(float) * 4 * (size_t)na + score_box_bytes(na); }
            if (rows_moving(rq[r].dst)) { ++pl.n_dirs; out_bytes += row_bytes * (size_t)na; pl.row_blocks = std::max(pl.row_blocks, row_blocks_of(na)); }
            if (rows_fixed(rq[r].dst)) { ++pl.n_dirs; out_bytes += row_bytes * (size_t)nb; pl.row_blocks = std::max(pl.row_blocks, row_blocks_of(nb)); }
        }
        const size_t heads = head_bytes * (size_t)pl.n_dirs;
        out_bytes += heads;
        const size_t off_box = sizeof(SupportMoveDesc) * (size_t)pl.n_moves, off_req = off_box + sizeof(BoxDesc) * (size_t)pl.n_moves;
        pl.tab_bytes = off_req + sizeof(Desc) * (size_t)pl.n_dirs;
        int rc;
        if ((rc = C.h_tab.ensure(pl.tab_bytes)) || (rc = C.d_tab.ensure(pl.tab_bytes)) || (rc = C.d_work.ensure(std::max(moved_bytes, (size_t)16)))) return rc;
        if (to_host && ((rc = C.d_out.ensure(out_bytes)) || (rc = C.h_out.ensure(out_bytes)))) return rc;
        if (to_host) C.out_bytes = out_bytes;
        unsigned char* const tab = static_cast<unsigned char*>(C.h_tab.p);
        SupportMoveDesc* const mv = reinterpret_cast<SupportMoveDesc*>(tab);
        BoxDesc* const bx = reinterpret_cast<BoxDesc*>(tab + off_box);
        Desc* const sd = reinterpret_cast<Desc*>(tab + off_req);
        std::memset(tab, 0, pl.tab_bytes);
        SideOut out{C, to_host, 0, heads};
        size_t moved_at = 0; int im = 0, id = 0;
        for (int r = 0; r < n; ++r) {
            const SideReq<Dst>& q = rq[r]; const Cloud& a = *q.a; const Cloud& b = *q.b;
            const PairState* from = q.from >= 0 ? static_cast<const PairState*>(d_states.p) + q.from : nullptr;
            const float* a_lo = a.rec(); const float* a_box = nullptr;
            if (q.tran || q.tran_from_state) {
                float* plane = reinterpret_cast<float*>(static_cast<unsigned char*>(C.d_work.p) + moved_at);
                float* gbox = plane + 4 * (size_t)a.n;
                moved_at += sizeof(float) * 4 * (size_t)a.n + score_box_bytes(a.n);
                SupportMoveDesc& M = mv[im]; BoxDesc& B = bx[im]; ++im;
                M.src = a.rec(); M.dst = plane; M.n = a.n; M.from = q.tran_from_state ? from : nullptr;
                for (int i = 0; i < 12; ++i) M.tran[i] = q.tran_from_state ? 0.f : q.tran[i];
                B.rec = plane; B.gbox = gbox; B.self_cache = score_self_cache(gbox, a.n); B.n = a.n; B.ngroups = score_groups(a.n);
                a_lo = plane; a_box = gbox;
            } else if (rows_fixed(q.dst)) {
                if ((rc = ensure_boxes(a, s))) return rc;
                a_box = static_cast<const float*>(a.boxes.p);
            }
            auto side = [&](const float* rows_lo, const Cloud& rows, const float* cols_lo, const Cloud& cols, const float* cols_box, bool swapped) {
                Desc& D = sd[id++];
                D.a_lo = rows_lo; D.a_hi = rows.rec() + hi_off(rows.n, 0); D.na = rows.n;
                D.b_lo = cols_lo; D.b_hi = cols.rec() + hi_off(cols.n, 0); D.nb = cols.n;
                D.bbox = cols_box; D.nbox = score_groups(cols.n);
                D.ell = q.ell; D.from = from;
                outputs(D, q.dst, swapped, (size_t)rows.n, out);
            };
            if (rows_moving(q.dst)) {
                if ((rc = ensure_boxes(b, s))) return rc;
                side(a_lo, a, b.rec(), b, static_cast<const float*>(b.boxes.p), false);
            }
            if (rows_fixed(q.dst)) side(b.rec(), b, a_lo, a, a_box, true);
        }
        const unsigned char* const dtab = static_cast<const unsigned char*>(C.d_tab.p);
        pl.d_mv = reinterpret_cast<const SupportMoveDesc*>(dtab); pl.d_bx = reinterpret_cast<const BoxDesc*>(dtab + off_box); pl.d_descs = dtab + off_req;
        return CVO_OK;
    }
    // One support or matches call from its checks to its end, on stream s (one call of a kind at a time: begin() waits for the one before).  what /
    // kernel: the kind as the messages name it; kind_check(dst): the kind's own check of a request, made between the clouds' and the transform's;
    // launch(plan, wgs_started, sweep_submitted): the kind's launcher.  The call ends as its form asks (side_publish): with an out_stream, the
    // stream the caller's device arrays are used on, that stream waits for it; else the host does, and to_host arrays are filled.
    template <class Desc, class Dst, class KindCheck, class Outputs, class Launch>
    int run_sides(SideCall& C, const SideReq<Dst>* rq, int n, hipStream_t s, bool to_host, hipStream_t out_stream, const char* what, const char* kernel,
                  size_t row_bytes, size_t head_bytes, int (*row_blocks_of)(int), KindCheck&& kind_check, Outputs&& outputs, Launch&& launch) {
        HIP_TRY(hipSetDevice(device));
        if (n <= 0) return fail(CVO_ERR_INVALID, std::string("bad ") + kernel + " request count");
        int rc;
        for (int r = 0; r < n; ++r) {
            if (!rq[r].a || !rq[r].b || rq[r].a->n <= 0 || rq[r].b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "empty cloud");
            if ((rc = kind_check(rq[r].dst))) return rc;
            if (!rows_moving(rq[r].dst) && !rows_fixed(rq[r].dst)) return fail(CVO_ERR_INVALID, std::string(what) + ": no output array");
            if (rq[r].tran_from_state && rq[r].from < 0) return fail(CVO_ERR_INVALID, std::string(what) + ": transform from a state that is not named");
        }
        SidePlan pl;
        if ((rc = C.begin(*this, s, false)) || (rc = build_sides<Desc>(C, rq, n, s, to_host, row_bytes, head_bytes, row_blocks_of, outputs, pl)) ||
            (rc = C.order_after(out_stream, s)) || (rc = C.upload(pl.tab_bytes, s))) return rc;
        const hipError_t e = counted_sweep((unsigned)pl.row_blocks * (unsigned)pl.n_dirs, [&](unsigned* wgs_started, bool* sweep_submitted) { return launch(pl, wgs_started, sweep_submitted); });
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string(kernel) + " kernel launch: " + hipGetErrorString(e));
        return (rc = C.finish(s)) ? rc : side_publish(C, out_stream);
    }
    // support: two arrays a direction, 8 bytes a row
    int point_sides(const SupportReq* rq, int n, hipStream_t s, bool to_host, hipStream_t out_stream = nullptr) {
        return run_sides<SupportDesc>(support_call, rq, n, s, to_host, out_stream, "point support", "support", 8, 0, support_row_blocks,
            [](const cvo_point_support_dst& d) {
                return !d.sum_moving != !d.count_moving || !d.sum_fixed != !d.count_fixed ? fail(CVO_ERR_INVALID, "point support: a direction needs its sum and its count array") : CVO_OK;
            },
            [](SupportDesc& D, const cvo_point_support_dst& d, bool swapped, size_t rows, SideOut& out) {
                D.sum = out.rows(swapped ? d.sum_fixed : d.sum_moving, 4 * rows); D.count = out.rows(swapped ? d.count_fixed : d.count_moving, 4 * rows);
            },
            [&](const SidePlan& pl, unsigned* wgs_started, bool* sweep_submitted) {
                return launch_support(pl.d_mv, pl.d_bx, pl.n_moves, pl.n_move_max, static_cast<const SupportDesc*>(pl.d_descs), pl.n_dirs, pl.row_blocks, P, s, wgs_started, sweep_submitted);
            });
    }
    // matches: five arrays a direction, 28 bytes a row, and, where dst.fit is given, a fit record per computed direction (24 bytes)
    int point_sides(const MatchReq* rq, int n, hipStream_t s, bool to_host, hipStream_t out_stream = nullptr) {
        bool with_fit = false;
        for (int r = 0; r < n; ++r) if (rq[r].dst.fit) with_fit = true;
        return run_sides<MatchDesc>(match_call, rq, n, s, to_host, out_stream, "point matches", "match", 28, sizeof(MatchFit), match_row_blocks,
            [](const cvo_point_matches_dst&) { return CVO_OK; },
            [](MatchDesc& D, const cvo_point_matches_dst& d, bool swapped, size_t rows, SideOut& out) {
                D.best = out.rows(swapped ? d.best_fixed : d.best_moving, 4 * rows); D.best_value = out.rows(swapped ? d.best_value_fixed : d.best_value_moving, 4 * rows);
                D.mean = out.rows(swapped ? d.mean_fixed : d.mean_moving, 12 * rows);
                D.sum = out.rows(swapped ? d.sum_fixed : d.sum_moving, 4 * rows); D.count = out.rows(swapped ? d.count_fixed : d.count_moving, 4 * rows);
                D.fit = d.fit ? reinterpret_cast<MatchFit*>(out.head(d.fit + (swapped ? 1 : 0), sizeof(MatchFit))) : nullptr;
            },
            [&](const SidePlan& pl, unsigned* wgs_started, bool* sweep_submitted) {
                return launch_match(pl.d_mv, pl.d_bx, pl.n_moves, pl.n_move_max, static_cast<const MatchDesc*>(pl.d_descs), pl.n_dirs, pl.row_blocks, with_fit, P, s, wgs_started, sweep_submitted);
            });
    }

    // Pose hypotheses (cvo_hypothesis_kernels.hip; include/cvo_hip.h: cvo_score_hypotheses) and pose models (cvo_pose_model_kernels.hip; cvo_pose_models):
    // for every request the moving cloud a under each of the k transforms trans[r][0 .. k) against the fixed cloud b at `ell`, all in ONE sweep launch,
    // and the reduce launch behind it.  What the two have in common between begin() and the launch: the table -- one Desc per pair, then the pairs' k
    // transforms each, copied from the caller's array before the call returns (trans null: none) -- the sweep's partials (`terms` doubles per pair,
    // transform and row block), the pinned block the kernels write their answers to, and per pair the clouds and the fixed cloud's boxes.
    // own(D, rq[r]) sets the kind's own fields.
    template <class Desc, class Req, class Own>
    int build_pairs(SideCall& C, const Req* rq, int n, int k, const float* trans, float ell, hipStream_t s, int (*row_blocks_of)(int), size_t terms, size_t answer_bytes,
                    Own&& own, SidePlan& pl) {
        for (int r = 0; r < n; ++r) pl.row_blocks = std::max(pl.row_blocks, row_blocks_of(rq[r].a->n));
        const size_t off_tran = sizeof(Desc) * (size_t)n;
        pl.tab_bytes = off_tran + (trans ? sizeof(float) * 12 * (size_t)n * k : 0);
        int rc;
        if ((rc = C.h_tab.ensure(pl.tab_bytes)) || (rc = C.d_tab.ensure(pl.tab_bytes)) || (rc = C.h_out.ensure(answer_bytes)) ||
            (rc = C.d_work.ensure(sizeof(double) * terms * (size_t)n * k * pl.row_blocks))) return rc;
        unsigned char* const tab = static_cast<unsigned char*>(C.h_tab.p);
        Desc* const descs = reinterpret_cast<Desc*>(tab);
        std::memset(tab, 0, off_tran);
        if (trans) std::memcpy(tab + off_tran, trans, sizeof(float) * 12 * (size_t)n * k);
        const float* const d_tran = reinterpret_cast<const float*>(static_cast<const unsigned char*>(C.d_tab.p) + off_tran);
        for (int r = 0; r < n; ++r) {
            const Cloud& a = *rq[r].a; const Cloud& b = *rq[r].b;
            if ((rc = ensure_boxes(b, s))) return rc;
            Desc& D = descs[r];
            D.a = a.rec(); D.na = a.n; D.b = b.rec(); D.nb = b.n;
            D.bbox = static_cast<const float*>(b.boxes.p); D.nbox = score_groups(b.n);
            D.trans = trans ? d_tran + 12 * (size_t)r * k : nullptr; D.ell = ell;
            if ((rc = own(D, rq[r]))) return rc;
        }
        pl.d_descs = C.d_tab.p;
        return CVO_OK;
    }
    // One hypothesis or pose-model call from its checks to the event behind its launches.  kind: as the messages name it; req_check(rq[r]): the kind's
    // own check of a request, after the clouds'; launch(plan, wgs_started, sweep_submitted): the kind's launcher.  s waits for an align launch on a
    // caller's stream; nothing waits for the device here but the call before.
    template <class Desc, class Req, class ReqCheck, class Own, class Launch>
    int run_pairs(SideCall& C, const Req* rq, int n, int k, const float* trans, float ell, hipStream_t s, const char* kind, int (*row_blocks_of)(int), size_t terms,
                  size_t answer_bytes, ReqCheck&& req_check, Own&& own, Launch&& launch) {
        HIP_TRY(hipSetDevice(device));
        if (n <= 0 || k < 1 || k > hyp_max()) return fail(CVO_ERR_INVALID, std::string("bad ") + kind + " request");
        int rc;
        for (int r = 0; r < n; ++r) {
            if (!rq[r].a || !rq[r].b || rq[r].a->n <= 0 || rq[r].b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "empty cloud");
            if ((rc = req_check(rq[r]))) return rc;
        }
        SidePlan pl;
        if ((rc = C.begin(*this, s, true)) || (rc = build_pairs<Desc>(C, rq, n, k, trans, ell, s, row_blocks_of, terms, answer_bytes, own, pl)) ||
            (rc = C.upload(pl.tab_bytes, s))) return rc;
        const hipError_t e = counted_sweep((unsigned)pl.row_blocks * (unsigned)k * (unsigned)n, [&](unsigned* wgs_started, bool* sweep_submitted) { return launch(pl, wgs_started, sweep_submitted); });
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string(kind) + " kernel launch: " + hipGetErrorString(e));
        return C.finish(s);
    }
    // Hypotheses.  seed: the select step also writes d_states[rq[r].state] -- R, T from reset_initial(best hypothesis), ell, transform and iter from
    // rq[r].start.
    struct HypReq { const Cloud* a; const Cloud* b; int state; const PairState* start; };
    int hyp_n = 0, hyp_k = 0;
    bool hyp_seed = false;                  // the call in flight is a seeding call: its answers are kept for cvo_batch_hypothesis_results (hyp_keep)
    std::vector<cvo_inn_p> seed_scores; std::vector<int> seed_best; int seed_n = 0, seed_k = 0;   // the last seeding call's answers, once it has been waited for
    // the call in flight has finished: a seeding call's answers move out of the pinned block the next call writes over (hyp_call.before_reuse:
    // begin() comes here before it frees the record)
    int hyp_keep() {
        if (!hyp_call.queued) return CVO_OK;
        int rc = hyp_call.wait(); if (rc) return rc;
        if (hyp_seed) {
            const cvo_inn_p* sc = static_cast<const cvo_inn_p*>(hyp_call.h_out.p);
            const int* bs = reinterpret_cast<const int*>(sc + (size_t)hyp_n * hyp_k);
            seed_scores.assign(sc, sc + (size_t)hyp_n * hyp_k); seed_best.assign(bs, bs + hyp_n);
            seed_n = hyp_n; seed_k = hyp_k; hyp_seed = false;
        }
        return CVO_OK;
    }
    int hyp_enqueue(const HypReq* rq, int n, int k, const float* trans, float ell, hipStream_t s, bool seed) {
        SideCall& C = hyp_call;
        int rc = run_pairs<HypDesc>(C, rq, n, k, trans, ell, s, "hypothesis", hyp_row_blocks, 2, sizeof(cvo_inn_p) * (size_t)n * k + sizeof(int) * (size_t)n,
            [](const HypReq&) { return CVO_OK; },
            [&](HypDesc& D, const HypReq& q) {
                if (!seed) return (int)CVO_OK;
                if (int rcs = d_states.ensure(sizeof(PairState) * (size_t)std::max(1, state_slots))) return rcs;   // (the size every launch asks for: it stays where it is)
                if (q.state < 0 || q.state >= state_slots || !q.start) return fail(CVO_ERR_INVALID, "hypothesis seed: no device state for the pair");
                D.state = static_cast<PairState*>(d_states.p) + q.state;
                D.seed_ell = q.start->ell; D.seed_iter = q.start->iter;
                std::memcpy(D.seed_transform, q.start->transform, sizeof(D.seed_transform));
                return (int)CVO_OK;
            },
            [&](const SidePlan& pl, unsigned* wgs_started, bool* sweep_submitted) {
                cvo_inn_p* const sc = static_cast<cvo_inn_p*>(C.h_out.p);
                return launch_hypotheses(static_cast<const HypDesc*>(pl.d_descs), n, k, pl.row_blocks, P, static_cast<double*>(C.d_work.p), reinterpret_cast<HypScore*>(sc),
                                         reinterpret_cast<int*>(sc + (size_t)n * k), seed ? 1 : 0, s, wgs_started, sweep_submitted);
            });
        if (rc) return rc;
        hyp_seed = seed; hyp_n = n; hyp_k = k;
        return CVO_OK;
    }
    // waits for the scores-only call queued last and hands out its answers (best may be null)
    int hyp_collect(cvo_inn_p* scores, int* best) {
        if (hyp_call.queued && hyp_seed) return fail(CVO_ERR_INVALID, hyp_call.none_queued);
        int rc = side_collect(hyp_call); if (rc) return rc;
        const cvo_inn_p* sc = static_cast<const cvo_inn_p*>(hyp_call.h_out.p);
        std::memcpy(scores, sc, sizeof(cvo_inn_p) * (size_t)hyp_n * hyp_k);
        if (best) std::memcpy(best, sc + (size_t)hyp_n * hyp_k, sizeof(int) * (size_t)hyp_n);
        return CVO_OK;
    }

    // Pose models: value, gradient and Hessian at each of the k transforms -- or, from >= 0 (k = 1, trans null), at the transform and ell of
    // d_states[from], so that the call can be queued behind the align launch that writes them.  Every call is collected before its entry point returns.
    struct PoseModelReq { const Cloud* a; const Cloud* b; int from; };
    int pm_n = 0, pm_k = 0;
    int pm_enqueue(const PoseModelReq* rq, int n, int k, const float* trans, float ell, hipStream_t s) {
        SideCall& C = pm_call;
        int rc = run_pairs<PoseModelDesc>(C, rq, n, k, trans, ell, s, "pose model", pose_model_row_blocks, POSE_MODEL_TERMS, sizeof(PoseModel) * (size_t)n * k,
            [&](const PoseModelReq& q) { return (q.from >= 0 ? (k != 1 || q.from >= state_slots) : !trans) ? fail(CVO_ERR_INVALID, "pose models: no transform for a pair") : CVO_OK; },
            [&](PoseModelDesc& D, const PoseModelReq& q) {
                if (q.from >= 0) { D.from = static_cast<const PairState*>(d_states.p) + q.from; D.trans = nullptr; }
                return (int)CVO_OK;
            },
            [&](const SidePlan& pl, unsigned* wgs_started, bool* sweep_submitted) {
                return launch_pose_models(static_cast<const PoseModelDesc*>(pl.d_descs), n, k, pl.row_blocks, P, static_cast<double*>(C.d_work.p), static_cast<PoseModel*>(C.h_out.p), s,
                                          wgs_started, sweep_submitted);
            });
        if (rc) return rc;
        pm_n = n; pm_k = k;
        return CVO_OK;
    }
    // waits for the call queued last and hands out its models
    int pm_collect(cvo_pose_model* out) {
        int rc = side_collect(pm_call); if (rc) return rc;
        std::memcpy(out, pm_call.h_out.p, sizeof(cvo_pose_model) * (size_t)pm_n * pm_k);
        return CVO_OK;
    }
};

// ---- host-side pieces of the reference's state helpers ----------------------
struct Aff { float m[12]; };
Aff aff_identity() { Aff a; std::memset(a.m, 0, sizeof(a.m)); a.m[0] = a.m[5] = a.m[10] = 1.f; return a; }
// (the arithmetic is stated once, in cvo_math.hpp: the device evaluates reset_initial too, cvo_track_link_kernel)
Aff aff_mul(const Aff& a, const Aff& b) { Aff c; aff_mul12(a.m, b.m, c.m); return c; }   // Affine3f * Affine3f

void sym_eig6(const double* Hin, double* ev) {   // cyclic Jacobi
    double A[36]; std::memcpy(A, Hin, sizeof(A));
    // (the eigenvalues are rounded to f32 by the caller, cvo.cpp:728: off-diagonal mass below 1e-30 of the diagonal's moves them by far less than half an ulp of
    //  that; running on until it underflowed took eight to ten sweeps instead of four or five -- 0.5 ms of host time per 64-pair score block)
    double diag2 = 0; for (int i = 0; i < 6; ++i) diag2 += A[i * 6 + i] * A[i * 6 + i];
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0; for (int i = 0; i < 6; ++i) for (int j = i + 1; j < 6; ++j) off += A[i * 6 + j] * A[i * 6 + j];
        if (off < 1e-300 || off <= 1e-30 * (diag2 + off)) break;
        for (int p = 0; p < 6; ++p) for (int q = p + 1; q < 6; ++q) {
            if (A[p * 6 + q] == 0.0) continue;
            const double theta = (A[q * 6 + q] - A[p * 6 + p]) / (2.0 * A[p * 6 + q]);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
            const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 6; ++k) { const double akp = A[k * 6 + p], akq = A[k * 6 + q]; A[k * 6 + p] = c * akp - s * akq; A[k * 6 + q] = s * akp + c * akq; }
            for (int k = 0; k < 6; ++k) { const double apk = A[p * 6 + k], aqk = A[q * 6 + k]; A[p * 6 + k] = c * apk - s * aqk; A[q * 6 + k] = s * apk + c * aqk; }
        }
    }
    for (int i = 0; i < 6; ++i) ev[i] = A[i * 6 + i];
}

// 21 upper-triangle terms -> 6x6 [[A, C^T],[C, D]] (cvo.cpp:700-704), then the
// scale / eigen-shift epilogue of se3_Hessian (cvo.cpp:726-758) in f32 as the reference.
void finish_hessian(const double* terms21, int inliers, double Hout[36]) {
    float H[36];
    if (inliers) {
        const double* t = terms21;
        float A3[9], C3[9], D3[9];
        A3[0] = (float)t[0]; A3[1] = A3[3] = (float)t[1]; A3[2] = A3[6] = (float)t[2]; A3[4] = (float)t[3]; A3[5] = A3[7] = (float)t[4]; A3[8] = (float)t[5];
        for (int i = 0; i < 9; ++i) C3[i] = (float)t[6 + i];
        D3[0] = (float)t[15]; D3[1] = D3[3] = (float)t[16]; D3[2] = D3[6] = (float)t[17]; D3[4] = (float)t[18]; D3[5] = D3[7] = (float)t[19]; D3[8] = (float)t[20];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) {
            H[r * 6 + c] = A3[r * 3 + c]; H[r * 6 + 3 + c] = C3[c * 3 + r]; H[(3 + r) * 6 + c] = C3[r * 3 + c]; H[(3 + r) * 6 + 3 + c] = D3[r * 3 + c];
        }
        const float scale = (float)(-1.0 / 100000);                 // cvo.cpp:727
        for (int i = 0; i < 36; ++i) H[i] = H[i] * scale;
        double Hd[36], evd[6]; for (int i = 0; i < 36; ++i) Hd[i] = H[i];
        sym_eig6(Hd, evd);
        float ev[6]; for (int i = 0; i < 6; ++i) ev[i] = (float)evd[i];
        auto min_abs = [&]() { int mi = 0; for (int i = 1; i < 6; ++i) if (std::fabs(ev[i]) < std::fabs(ev[mi])) mi = i; return ev[mi]; };
        float sufficient_scale = 0.0f, min_eigen = min_abs();
        int guard = 0;
        while (std::fabs(min_eigen) < 1.0 && guard++ < 1000) {      // cvo.cpp:740-746
            sufficient_scale += (float)(1.0 - min_eigen);
            for (int i = 0; i < 6; ++i) ev[i] += (float)(1.0 - min_eigen) * 1.0f;
            min_eigen = min_abs();
        }
        for (int i = 0; i < 6; ++i) H[i * 6 + i] += sufficient_scale * 1.0f;   // cvo.cpp:747
    } else {
        for (int i = 0; i < 36; ++i) H[i] = (i % 7 == 0) ? 1.f : 0.f;         // cvo.cpp:755
    }
    for (int i = 0; i < 36; ++i) Hout[i] = (double)H[i];                      // cvo.cpp:758
}

}  // namespace

// =============================================================================
struct cvo_handle_s {
    cvo_params prm;
    Engine eng;
    std::shared_ptr<Cloud> fixed, moving, previous;     // ptr_fixed_pcd / ptr_moving_pcd / ptr_previous_pcd, cvo.hpp:91-94 (shared with last_generated() only: never written again)
    bool pre_pc_init = false, init = false, first_frame = true;
    int num_fixed = 0, num_moving = 0;
    float R[9], T[3], ell;
    Aff transform, prev_transform, accum_transform;
    int iter = 0, A_nonzero = 0;
    int num_want = 3000;                                             // pcd_generator.cpp:22
    Cloud scratch_a, scratch_b;                                      // host clouds handed to function_inner_product / se3_Hessian directly
    // The tracker calls compute_innerproduct(tran = the transform it has just been given) right behind every match_* (local_tracker.cpp:356-375, 415-431): with
    // cvo_set_tail_scores(h, 1) the align launch answers that block in its tail (Engine::tail_scores) and the answers wait here for the call -- valid for
    // exactly these clouds, this ell and this transform; anything else goes to the score kernel as before.  Off by default: one pair alone runs on eight cooperating
    // workgroups, whose tail (a transform, a cull, two list walks, five exchanges) costs the launch 0.12 ms where the score launch behind it costs 0.07-0.10
    // (profiles/r04_tracker_path.txt); batches, one workgroup per pair with every CU busy, are where it pays (cvo_batch_set_tail_scores).
    // What "answers" means for a handle (CVO_HIP_HANDLE_TAIL=queue|kernel, default queue): the score kernel for {mv, fx, the result's transform and ell} is QUEUED right behind the
    // align kernel, before the host starts waiting for the alignment (transform and ell come from the device-resident state, as cvo_batch_enqueue_innerproduct has it);
    // cvo_align returns when the alignment is in, the score kernel runs while the caller looks at the transform, and compute_innerproduct(tran = that transform) only
    // collects.  "kernel" is the batches' way (the align launch's own tail), slower for one pair on eight workgroups (above).
    // cvo_set_tail_scores: 0 never, 1 always, 2 (default) when the handle's previous alignment was followed by exactly that question -- the tracker's two objects are asked
    // after every frame (local_tracker.cpp:375, 431) and queue from their second frame on; a loop-closure object (compute_innerproduct_lc) never does.
    int tail_mode = 2;
    bool asked_after_align = false;                                  // compute_innerproduct(tran = the last alignment's transform) came since that alignment
    bool tail_scores = false;                                        // this alignment starts the block (decided per alignment from the two above)
    bool tail_in_kernel = false;
    bool queued_valid = false;                                       // a score block for (queued_fixed, queued_moving, h->transform, h->ell) is queued or done on eng.score_stream
    const Cloud* queued_fixed = nullptr; const Cloud* queued_moving = nullptr; float queued_ell = 0.f, queued_tran[12];
    int queued_hits = 0;                                             // score blocks answered by what an alignment had queued
    int shared_hits = 0;                                             // clouds this handle took from last_generated() instead of generating them
    int staged_hits = 0;                                             // clouds this handle took from a generation started ahead of time (cvo_stage_next_frame)
    bool tail_valid = false;
    double tail_r[5][24];
    const Cloud* tail_fixed = nullptr; const Cloud* tail_moving = nullptr;
    float tail_ell = 0.f, tail_tran[12];
};

// Scratch of cvo_batch_set_pairs_images: every buffer holds n_cap images of w x h one behind the other (the strides of cvo_pcd_kernels.hip),
// and one slot of PCD_CLOUD_CAP points per image for its cloud.  Grows with the largest call, released by cvo_batch_destroy.
constexpr int PCD_CLOUD_CAP = 65535;
struct BatchImages {
    DevBuf bgr, depth, I0, I1, I2, dx0, dy0, abs0, abs1, abs2, ths, thsS, map, pattern, tiles, rec, cloud, px, cams;
    PinBuf stage, h_rec, h_cams;
    PinBuf h_ingest;                                                // device images: the ingest kernel's descriptor table (read by the kernel where it is)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;                   // ... and the two edges between the caller's image_stream and the stream of the ingest
    int n_cap = 0, w = 0, h = 0;
    int num_want = 3000;                                            // pcd_generator::num_want (pcd_generator.cpp:22)
    void release() {
        for (DevBuf* b : {&bgr, &depth, &I0, &I1, &I2, &dx0, &dy0, &abs0, &abs1, &abs2, &ths, &thsS, &map, &pattern, &tiles, &rec, &cloud, &px, &cams}) b->release();
        stage.release(); h_rec.release(); h_cams.release(); h_ingest.release();
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
        ev_in = ev_out = nullptr;
        n_cap = w = h = 0;
    }
};

// What the hand-over of caller-owned device clouds needs (cvo_*_device_clouds): the ingest kernel's descriptor table and the table its blocks write
// their cost samples to (pinned, free again once ev_out has been waited for), the two edges between the caller's cloud_stream and the engine's
// stream, and the box launch's descriptor table -- two of them taken in turn, since the host waits for the ingest and not for the boxes behind it.
struct CloudIntake {
    PinBuf h_desc, h_cost, h_box[2];
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_box[2] = {nullptr, nullptr};
    bool box_queued[2] = {false, false}; int flip = 0;
    void release() {
        h_desc.release(); h_cost.release(); h_box[0].release(); h_box[1].release();
        for (hipEvent_t* e : {&ev_in, &ev_out, &ev_box[0], &ev_box[1]}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
        box_queued[0] = box_queued[1] = false;
    }
};

// The frames of the NEXT step of a batch's or a tracker's streams, generated ahead of it (cvo_batch_stage_images, cvo_tracks_stage_async) on a stream
// and in generator scratch of their own, while the launches of the current step run.  Three states: nothing staged; `pending`, the generator
// queued (ev_gen behind its read-back of the point counts); `placed`, the counts read, every cloud copied into a cloud object that nothing
// else holds and its group boxes made (one scatter and ONE box launch on the stage stream, ev_done behind them).  Placing needs the counts
// on the host, so it happens where the host next looks and finds the generator finished: at the end of a wait, else in the consuming call.
struct FrameStage {
    hipStream_t s = nullptr; hipEvent_t ev_gen = nullptr, ev_done = nullptr;
    BatchImages img;
    PinBuf h_box;                                                   // the box launch's descriptor table (read by the kernel where it is)
    bool pending = false, placed = false, gen_waited = true;
    int rc = CVO_OK; std::string err;                               // what placing found: reported by the consuming call
    std::vector<int> list, points;                                  // the slots / streams listed, in list order, and their clouds' points
    std::vector<std::shared_ptr<Cloud>> clouds;
    std::vector<std::shared_ptr<Cloud>>* pool = nullptr;            // where free cloud objects come from: one that only the pool holds is free
    long long taken = 0;
};

// A pair slot run as one cvo::cvo odometry object (cvo_batch_advance_images): the fields a handle carries from one align() into the next
// (cvo_handle_s, do_align), kept on the host and uploaded as the slot's start state by every launch that lists it.
struct StreamSlot {
    bool on = false;                        // the slot is a stream (else a plain pair)
    bool init = false;                      // its first frame is in: the FIXED cloud (cvo.cpp:352-360)
    bool has_moving = false;                // a later frame is in: the MOVING cloud, possibly empty
    float R[9], T[3], ell;
    int iter = 0;
    Aff transform, prev_transform, accum_transform;
};

struct cvo_batch_s {
    cvo_params prm;
    Engine eng;
    int max_pairs = 0;
    std::vector<std::shared_ptr<Cloud>> fixed, moving;        // (shared: a tracker stream's frame is held by its odometry and its keyframe object at once, cvo_tracks_s)
    BatchImages img;
    CloudIntake cin;
    std::vector<PairState> init_states;     // what set_pair / set_state last gave
    std::vector<unsigned char> dirty;       // per slot: the plain pair's device state differs from init_states (set for every slot by any set_*, as one flag was)
    std::vector<StreamSlot> streams;
    int last_n = 0;
    std::vector<int> last_slots;            // the slot of every position of the last launch (positions = the caller's list order)
    std::vector<unsigned char> last_stream_pos, last_not_run;   // ... which were stream slots, which had no moving cloud (not run: CVO_ERR_NOT_INITIALIZED)
    bool settled = true;                    // the last launch's results have been taken in (batch_settle)
    bool clouds_changed = false;            // a slot of the last launch has new clouds since: answers computed from its clouds would be for others
    FrameStage stage;                       // the next frames, staged ahead (cvo_batch_stage_images; a tracker's stage lives in its odometry batch)
    std::vector<std::shared_ptr<Cloud>> pool;   // cloud objects for staged frames and the ones slots gave back to cvo_batch_advance_staged
};

namespace {
Cloud* slot_cloud(cvo_handle_s* h, int slot) {
    switch (slot) { case CVO_SLOT_FIXED: return h->fixed.get(); case CVO_SLOT_MOVING: return h->moving.get(); case CVO_SLOT_PREVIOUS: return h->previous.get(); }
    return nullptr;
}
void slots_changed(cvo_handle_s* h) { h->tail_valid = false; h->queued_valid = false; }   // answers held for the clouds that were there are void (a new cloud may live at an old one's address)
std::shared_ptr<Cloud>& slot_to_fill(cvo_handle_s* h) {            // cvo.cpp:352-366: the first cloud is the FIXED one, every later one MOVING
    slots_changed(h);
    if (!h->init) { if (!h->fixed || h->fixed.use_count() > 1 || h->fixed->n > 0) h->fixed = std::make_shared<Cloud>(); return h->fixed; }
    h->moving = std::make_shared<Cloud>();
    return h->moving;
}
void fresh_state(PairState& s, float ell) {
    std::memset(&s, 0, sizeof(s));
    s.R[0] = s.R[4] = s.R[8] = 1.f; s.ell = ell;
    s.transform[0] = s.transform[5] = s.transform[10] = 1.f;
}
// the start state of an alignment from the fields an odometry object carries (cvo_handle_s, cvo_batch_s::streams)
void carried_state(PairState& st, const float R[9], const float T[3], float ell, int iter, const Aff& transform) {
    fresh_state(st, ell);
    std::memcpy(st.R, R, sizeof(st.R)); std::memcpy(st.T, T, sizeof(st.T));
    st.iter = iter;
    std::memcpy(st.transform, transform.m, sizeof(st.transform));
}
int do_align(cvo_handle_s* h, cvo_trace_row* trace, int trace_cap, int* trace_len) {
    if (trace_len) *trace_len = 0;
    if (!h->fixed || !h->moving || h->fixed->n <= 0 || h->moving->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "align: empty fixed or moving cloud");
    PairState st; carried_state(st, h->R, h->T, h->ell, h->iter, h->transform);
    std::vector<Engine::PairIn> pairs{{h->fixed.get(), h->moving.get()}};
    const bool want_trace = trace && trace_cap > 0;
    h->tail_valid = false; h->queued_valid = false;
    h->tail_scores = h->tail_mode == 1 || (h->tail_mode == 2 && h->asked_after_align);
    h->asked_after_align = false;
    h->eng.tail_scores = h->tail_scores && h->tail_in_kernel;
    int rc = h->eng.launch(pairs, &st, true, nullptr, want_trace, trace_cap); if (rc) return rc;
    if (want_trace) {
        // results copy is already queued; queue the trace copies behind it on the same stream
        HIP_TRY(hipMemcpyAsync(trace, h->eng.d_trace.p, sizeof(TraceRow) * trace_cap, hipMemcpyDeviceToHost, h->eng.stream));
        HIP_TRY(hipMemcpyAsync(trace_len, h->eng.d_tracelen.p, sizeof(int), hipMemcpyDeviceToHost, h->eng.stream));
    }
    bool queued = false;
    if (h->tail_scores && !h->tail_in_kernel && !want_trace) {       // the tracker's score block (cvo.cpp:489-500) behind the align kernel, transform and ell from the pair's state
        const Cloud* fx = h->fixed.get(); const Cloud* mv = h->moving.get();
        const Engine::ScoreReq rq[5] = {{mv, nullptr, fx, false, 0.f, 0, false}, {mv, nullptr, fx, false, 0.f, 0, true}, {fx, nullptr, fx, false, 0.f, 0, false},
                                        {mv, nullptr, mv, false, 0.f, 0, false}, {mv, nullptr, fx, true, 0.f, 0, true}};
        queued = h->eng.score_enqueue(rq, 5, h->eng.last_stream) == CVO_OK;
    }
    rc = queued ? h->eng.wait_align_only() : h->eng.wait(); if (rc) { h->eng.score_pending = 0; return rc; }
    const PairState& r = h->eng.results()[0];
    if (r.status != CVO_OK) {
        // the block queued behind a FAILED alignment was computed from that alignment's device state: it answers nobody's question.  Let it leave the
        // device (the next score launch reuses its buffers) and drop it; the handle keeps the transform and ell of the alignment before.
        if (queued) { (void)hipStreamSynchronize(h->eng.last_stream); h->eng.score_pending = 0; }
        return fail(r.status, "align kernel reported an error (6 = inter-workgroup wait timed out)");
    }
    if (queued) { h->queued_valid = true; h->queued_fixed = h->fixed.get(); h->queued_moving = h->moving.get(); }   // (ell and transform: below, from the result)
    std::memcpy(h->R, r.R, sizeof(h->R)); std::memcpy(h->T, r.T, sizeof(h->T));
    h->ell = r.ell; h->iter = r.iter; h->A_nonzero = r.A_nonzero;
    Aff prev; std::memcpy(prev.m, r.prev_transform, sizeof(prev.m));
    h->prev_transform = prev;                                        // cvo.cpp:815
    h->accum_transform = aff_mul(h->accum_transform, prev);          // cvo.cpp:816
    std::memcpy(h->transform.m, r.transform, sizeof(float) * 12);    // update_tf, cvo.cpp:817
    if (h->queued_valid) { h->queued_ell = h->ell; std::memcpy(h->queued_tran, h->transform.m, sizeof(h->queued_tran)); }
    if (h->eng.last_tail) {                                           // the score block this launch answered in its tail, for the compute_innerproduct that follows
        std::memcpy(h->tail_r, h->eng.h_tail.p, sizeof(h->tail_r));
        h->tail_fixed = h->fixed.get(); h->tail_moving = h->moving.get(); h->tail_ell = h->ell;
        std::memcpy(h->tail_tran, h->transform.m, sizeof(h->tail_tran));
        h->tail_valid = true;
    }
    return CVO_OK;
}
}  // namespace

extern "C" {

const char* cvo_last_error(void) { return g_err.c_str(); }

int cvo_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < count; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

int cvo_default_params(cvo_params* p) {
    if (!p) return fail(CVO_ERR_INVALID, "null params");
    p->ell = 0.15; p->sigma = 0.1; p->sp_thres = 8e-3; p->c = 7.0; p->d = 7.0; p->c_ell = 200; p->c_sigma = 1;
    p->max_iter = 2000; p->min_step = 2 * 1.0e-1; p->eps = 5 * 1.0e-5; p->eps_2 = 1.0e-5;
    return CVO_OK;
}

int cvo_create(const cvo_params* p, int device, cvo_handle* out) {
    if (!out) return fail(CVO_ERR_INVALID, "null out");
    *out = nullptr;
    std::unique_ptr<cvo_handle_s> h(new cvo_handle_s());
    if (p) h->prm = *p; else cvo_default_params(&h->prm);
    int rc = h->eng.init(device, h->prm); if (rc) { h->eng.destroy(); return rc; }   // whatever init had created before it failed
    h->fixed.reset(new Cloud());                                     // ptr_fixed_pcd(new point_cloud), cvo.cpp:30
    h->ell = h->prm.ell;
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(h->R, I, sizeof(I)); h->T[0] = h->T[1] = h->T[2] = 0;  // cvo.cpp:66-67
    h->transform = h->prev_transform = h->accum_transform = aff_identity();   // cvo.cpp:68-70
    *out = h.release();
    return CVO_OK;
}

int cvo_destroy(cvo_handle h) {
    if (!h) return CVO_OK;
    (void)hipSetDevice(h->eng.device);
    if (h->eng.stream) (void)hipStreamSynchronize(h->eng.stream);
    h->fixed.reset(); h->moving.reset(); h->previous.reset();
    h->eng.destroy();
    delete h;
    return CVO_OK;
}

int cvo_set_pcd(cvo_handle h, const float* xyz, const float* feat, int n) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    const bool first = !h->init;
    std::shared_ptr<Cloud>& c = slot_to_fill(h);
    int rc = h->eng.upload(*c, xyz, feat, n); if (rc) return rc;
    if (first) { h->init = true; return CVO_OK; }                    // cvo.cpp:352-360
    h->num_fixed = h->fixed ? h->fixed->n : 0; h->num_moving = h->moving->n;   // cvo.cpp:370-371
    h->A_nonzero = 0;                                                // cvo.cpp:385
    return CVO_OK;
}

int cvo_set_tail_scores(cvo_handle h, int on) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (on < 0 || on > 2) return fail(CVO_ERR_INVALID, "cvo_set_tail_scores: 0 (never), 1 (always) or 2 (when the previous alignment was asked)");
    h->tail_mode = on; h->asked_after_align = false;
    if (const char* e = std::getenv("CVO_HIP_HANDLE_TAIL")) h->tail_in_kernel = std::strcmp(e, "kernel") == 0;
    if (!on) slots_changed(h);
    return CVO_OK;
}
int cvo_set_num_want(cvo_handle h, int num_want) {
    if (!h || num_want <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    h->num_want = num_want; return CVO_OK;
}

namespace {
// The frame this thread's last cloud was generated from, byte for byte?  Then `c` becomes a device copy of that cloud (positions + features, selected pixels:
// 100 KB at 3 k points, queued on the handle's stream) and nothing is generated: 0.22 ms -> the compare of 1.5 MB the staging copy would have read anyway.
// A different frame differs within the first bytes and costs nothing.
int take_from(const LastGenerated& g, cvo_handle_s* h, Cloud& c, const unsigned char* bgr8, const unsigned short* depth16, int w, int hh, const cvo_camera& cam, bool* taken) {
    *taken = false;
    if (!g.cloud || !g.stage || g.device != h->eng.device || g.w != w || g.h != hh || g.num_want != h->num_want ||
        std::memcmp(&g.cam, &cam, sizeof(cam)) != 0 || !bgr8 || !depth16) return CVO_OK;
    const size_t n = (size_t)w * hh;
    {
        std::lock_guard<std::mutex> lk(g.stage->mu);
        if (g.stage->stamp.load(std::memory_order_acquire) != g.stamp || g.stage->buf.bytes < 5 * n) return CVO_OK;
        const unsigned char* st = static_cast<const unsigned char*>(g.stage->buf.p);
        if (std::memcmp(st, bgr8, 3 * n) != 0 || std::memcmp(st + 3 * n, depth16, 2 * n) != 0) return CVO_OK;
    }
    const Cloud& src = *g.cloud;
    HIP_TRY(hipSetDevice(h->eng.device));
    c.n = src.n; c.n_px = src.n_px; c.cost_hint = src.cost_hint; c.boxes_valid = false; c.raw = nullptr;
    if (src.n > 0) {
        int rc = c.buf.ensure((size_t)src.n * REC * sizeof(float)); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c.buf.p, src.buf.p, (size_t)src.n * REC * sizeof(float), hipMemcpyDeviceToDevice, h->eng.stream));
    }
    if (src.n_px > 0) {
        int rc = c.px.ensure((size_t)src.n_px * 2 * sizeof(uint16_t)); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c.px.p, src.px.p, (size_t)src.n_px * 2 * sizeof(uint16_t), hipMemcpyDeviceToDevice, h->eng.stream));
    }
    HIP_TRY(hipStreamSynchronize(h->eng.stream));                    // complete when the call returns, as a generated cloud is (any stream may read it next)
    *taken = true;
    return CVO_OK;
}
int take_generated(cvo_handle_s* h, Cloud& c, const unsigned char* bgr8, const unsigned short* depth16, int w, int hh, const cvo_camera& cam, bool* taken) {
    *taken = false;
    if (!share_generated_clouds()) return CVO_OK;
    const int rc = take_from(last_generated(), h, c, bgr8, depth16, w, hh, cam, taken);
    if (rc == CVO_OK && *taken) ++h->shared_hits;
    return rc;
}

// ---- the NEXT frame's cloud, generated ahead of its set_pcd (cvo_stage_next_frame).  The reference's tracker handles a frame strictly in sequence
// (local_tracker.cpp:356 set_pcd + align, :375 scores, :415 set_pcd + align, :431 scores) and its generator is the first thing each frame waits for; frame t + 1's
// images do not depend on frame t's alignment, so a caller that has them early hands them over here and goes on with frame t: a worker thread with an engine of
// its own (own stream, own scratch) runs the generator beside the alignment -- eight workgroups of 256 CUs --, and cvo_set_pcd_images finds the finished cloud by
// comparing the images byte for byte, as it does for the second object of a frame.  One staged frame per host thread; the images must stay as they are until the
// cvo_set_pcd_images that takes them (or the next cvo_stage_next_frame) has returned.
struct FrameStager {
    Engine eng; bool ready = false;
    std::thread th; std::mutex mu; std::condition_variable cv;
    bool quit = false, busy = false, have = false;
    const unsigned char* bgr = nullptr; const unsigned short* depth = nullptr; int w = 0, h = 0, num_want = 0; cvo_camera cam{};
    LastGenerated out;              // valid when `have`: the staged frame and its cloud
    std::shared_ptr<ImageStage> stages[2]; int flip = 0;
    int rc = CVO_OK; std::string err;
    int start(int device, const cvo_params& prm) {
        const int r = eng.init(device, prm); if (r) return r;
        ready = true;
        th = std::thread([this] { run(); });
        return CVO_OK;
    }
    void run() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [this] { return quit || busy; });
            if (quit) return;
            lk.unlock();
            auto cloud = std::make_shared<Cloud>();
            // two stages in turn: the frame staged before this one has just been taken (or is about to be), and its second object still compares against ITS images
            if (!stages[flip]) stages[flip] = std::make_shared<ImageStage>();
            eng.img_stage = stages[flip]; flip ^= 1;
            const int r = eng.generate_pcd(*cloud, bgr, depth, w, h, cam, num_want);
            std::string e = r ? g_err : std::string();
            lk.lock();
            rc = r; err = e; have = (r == CVO_OK);
            if (have) {
                out.stage = eng.img_stage; out.stamp = out.stage->stamp.load(std::memory_order_acquire);
                out.device = eng.device; out.w = w; out.h = h; out.num_want = num_want; out.cam = cam; out.cloud = cloud;
            } else out.cloud.reset();
            busy = false;
            cv.notify_all();
        }
    }
    void wait_idle() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return !busy; }); }
    ~FrameStager() {
        if (ready) {
            { std::lock_guard<std::mutex> lk(mu); quit = true; }
            cv.notify_all();
            if (th.joinable()) th.join();
            out.cloud.reset();
            eng.destroy();
        }
    }
};
struct StagerOwner { FrameStager* p = nullptr; ~StagerOwner() { delete p; } };
FrameStager* frame_stager(int device, const cvo_params& prm, int* rc_out) {
    static thread_local StagerOwner own;
    *rc_out = CVO_OK;
    if (own.p && own.p->eng.device != device) { delete own.p; own.p = nullptr; }
    if (!own.p) {
        own.p = new FrameStager();
        const int rc = own.p->start(device, prm);
        if (rc) { delete own.p; own.p = nullptr; *rc_out = rc; }
    }
    frame_stager_slot() = own.p;
    return own.p;
}
}  // namespace

int cvo_set_pcd_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera* cam) {
    if (!h || !cam) return fail(CVO_ERR_INVALID, "null argument");
    const bool first = !h->init;
    std::shared_ptr<Cloud>& c = slot_to_fill(h);
    bool taken = false;
    int rc = take_generated(h, *c, bgr8, depth16, width, height, *cam, &taken); if (rc) return rc;
    if (!taken) {
        if (FrameStager* fs = frame_stager_slot()) {                  // a frame staged ahead (cvo_stage_next_frame)?  wait for its generation, then compare
            fs->wait_idle();
            if (fs->have) {
                rc = take_from(fs->out, h, *c, bgr8, depth16, width, height, *cam, &taken); if (rc) return rc;
                if (taken) {
                    ++h->staged_hits;
                    if (share_generated_clouds()) last_generated() = fs->out;   // the frame's second object finds it where it looks (take_generated)
                    fs->have = false; fs->out.cloud.reset();
                }
            }
        }
    }
    if (!taken) {
        LastGenerated& g = last_generated();
        g.cloud.reset();                                             // (frees the previous frame's cloud unless a handle still holds it)
        rc = h->eng.generate_pcd(*c, bgr8, depth16, width, height, *cam, h->num_want); if (rc) return rc;
        if (share_generated_clouds()) {
            g.stage = h->eng.img_stage; g.stamp = g.stage->stamp.load(std::memory_order_acquire);
            g.device = h->eng.device; g.w = width; g.h = height; g.num_want = h->num_want; g.cam = *cam; g.cloud = c;
        }
    }
    if (first) { h->init = true; return CVO_OK; }                    // cvo.cpp:352-360
    h->num_fixed = h->fixed ? h->fixed->n : 0; h->num_moving = h->moving->n;   // cvo.cpp:370-371
    h->A_nonzero = 0;                                                // cvo.cpp:385
    return CVO_OK;
}
int cvo_stage_next_frame(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera* cam) {
    if (!h || !cam || !bgr8 || !depth16) return fail(CVO_ERR_INVALID, "null argument");
    if (width < 64 || height < 64 || (size_t)width * height > (size_t)1 << 26) return fail(CVO_ERR_INVALID, "image size out of range");
    int rc = CVO_OK;
    FrameStager* fs = frame_stager(h->eng.device, h->prm, &rc);
    if (!fs) return rc;
    fs->wait_idle();                                                  // (a frame staged before and never asked for: dropped)
    {
        std::lock_guard<std::mutex> lk(fs->mu);
        fs->have = false; fs->out.cloud.reset();
        fs->bgr = bgr8; fs->depth = depth16; fs->w = width; fs->h = height; fs->num_want = h->num_want; fs->cam = *cam;
        fs->busy = true;
    }
    fs->cv.notify_all();
    return CVO_OK;
}
int cvo_staged_frame_count(cvo_handle h, int* count) { if (!h || !count) return fail(CVO_ERR_INVALID, "null argument"); *count = h->staged_hits; return CVO_OK; }
int cvo_queued_score_count(cvo_handle h, int* count) { if (!h || !count) return fail(CVO_ERR_INVALID, "null argument"); *count = h->queued_hits; return CVO_OK; }
int cvo_shared_cloud_count(cvo_handle h, int* count) { if (!h || !count) return fail(CVO_ERR_INVALID, "null argument"); *count = h->shared_hits; return CVO_OK; }

namespace {
// a cloud back to the reference layout on the host (cvo_get_cloud, cvo_batch_get_cloud), queued on the engine's stream behind whatever wrote it
int download_cloud(Engine& E, const Cloud* c, float* xyz, float* feat, int cap, int* n) {
    *n = c ? c->n : 0;
    if (!c || c->n == 0 || cap < c->n) return CVO_OK;
    if (!xyz || !feat) return fail(CVO_ERR_INVALID, "null output array");
    HIP_TRY(hipSetDevice(E.device));
    DevBuf tmp; int rc = tmp.ensure(sizeof(float) * 8 * (size_t)c->n); if (rc) return rc;
    float* dx = static_cast<float*>(tmp.p); float* df = dx + 3 * (size_t)c->n;
    hipError_t e = pcd_launch_unpack(c->rec(), c->n, dx, df, E.stream);
    if (e != hipSuccess) { tmp.release(); return fail(CVO_ERR_HIP, std::string("unpack kernel: ") + hipGetErrorString(e)); }
    hipError_t e1 = hipMemcpyAsync(xyz, dx, sizeof(float) * 3 * (size_t)c->n, hipMemcpyDeviceToHost, E.stream);
    hipError_t e2 = hipMemcpyAsync(feat, df, sizeof(float) * 5 * (size_t)c->n, hipMemcpyDeviceToHost, E.stream);
    hipError_t e3 = hipStreamSynchronize(E.stream);
    tmp.release();
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(CVO_ERR_HIP, "cloud download failed");
    return CVO_OK;
}
int download_selected_points(Engine& E, const Cloud* c, unsigned short* px, int cap, int* n) {
    *n = c ? c->n_px : 0;
    if (!c || c->n_px == 0 || cap < c->n_px) return CVO_OK;
    if (!px) return fail(CVO_ERR_INVALID, "null output array");
    HIP_TRY(hipSetDevice(E.device));
    HIP_TRY(hipMemcpyAsync(px, c->px.p, sizeof(unsigned short) * 2 * (size_t)c->n_px, hipMemcpyDeviceToHost, E.stream));
    HIP_TRY(hipStreamSynchronize(E.stream));
    return CVO_OK;
}
}  // namespace

int cvo_get_cloud(cvo_handle h, int slot, float* xyz, float* feat, int cap, int* n) {
    if (!h || !n) return fail(CVO_ERR_INVALID, "null argument");
    return download_cloud(h->eng, slot_cloud(h, slot), xyz, feat, cap, n);
}

int cvo_get_selected_points(cvo_handle h, int slot, unsigned short* px, int cap, int* n) {
    if (!h || !n) return fail(CVO_ERR_INVALID, "null argument");
    return download_selected_points(h->eng, slot_cloud(h, slot), px, cap, n);
}

int cvo_align_traced(cvo_handle h, cvo_trace_row* trace, int trace_cap, int* trace_len) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (trace && !trace_len) return fail(CVO_ERR_INVALID, "trace_len required with trace");
    return do_align(h, trace, trace_cap, trace_len);
}
int cvo_align(cvo_handle h) { return cvo_align_traced(h, nullptr, 0, nullptr); }

int cvo_match_odometry(cvo_handle h, const float* xyz, const float* feat, int n, double transform_out[12]) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (!h->init) return fail(CVO_ERR_NOT_INITIALIZED, "cvo not initialized !");    // cvo.cpp:463-466
    int rc = cvo_set_pcd(h, xyz, feat, n); if (rc) return rc;
    rc = cvo_align(h); if (rc) return rc;
    if (transform_out) for (int i = 0; i < 12; ++i) transform_out[i] = (double)h->transform.m[i];   // cvo.cpp:472
    return CVO_OK;
}
int cvo_match_odometry_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera* cam,
                              double transform_out[12]) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (!h->init) return fail(CVO_ERR_NOT_INITIALIZED, "cvo not initialized !");    // cvo.cpp:463-466
    int rc = cvo_set_pcd_images(h, bgr8, depth16, width, height, cam); if (rc) return rc;
    rc = cvo_align(h); if (rc) return rc;
    if (transform_out) for (int i = 0; i < 12; ++i) transform_out[i] = (double)h->transform.m[i];   // cvo.cpp:472
    return CVO_OK;
}
int cvo_match_keyframe_images(cvo_handle h, const unsigned char* bgr8, const unsigned short* depth16, int width, int height, const cvo_camera* cam,
                              double transform_out[12]) {
    return cvo_match_odometry_images(h, bgr8, depth16, width, height, cam, transform_out);   // cvo.cpp:563-576 is the same body
}
int cvo_match_keyframe(cvo_handle h, const float* xyz, const float* feat, int n, double transform_out[12]) {
    return cvo_match_odometry(h, xyz, feat, n, transform_out);       // cvo.cpp:563-576 is the same body
}

namespace {
void finish_inn_p(const double r[24], cvo_inn_p* out) {
    double sum = r[1]; if (sum == 0) sum = 1;                        // cvo.cpp:455-456
    out->value = (float)r[0]; out->num = (int)sum; out->num_e = 0;   // cvo.cpp:457
}
}  // namespace

int cvo_function_inner_product(cvo_handle h, int slot_a, const float* tran_a, int slot_b, cvo_inn_p* out) {
    if (!h || !out) return fail(CVO_ERR_INVALID, "null argument");
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "function_inner_product: empty cloud slot");
    double r[1][24];
    const Engine::ScoreReq rq[1] = {{a, tran_a, b, false, h->ell}};
    int rc = h->eng.score_many(rq, 1, r); if (rc) return rc;
    finish_inn_p(r[0], out);
    return CVO_OK;
}

int cvo_se3_hessian(cvo_handle h, int slot_a, const float* tran_a, int slot_b, double H[36], int* inliers) {
    if (!h || !H || !inliers) return fail(CVO_ERR_INVALID, "null argument");
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "se3_Hessian: empty cloud slot");
    double r[1][24];
    const Engine::ScoreReq rq[1] = {{a, tran_a, b, true, h->ell}};
    int rc = h->eng.score_many(rq, 1, r); if (rc) return rc;
    *inliers += (int)r[0][1];                                        // cvo.cpp:708 increments the caller's variable
    finish_hessian(r[0] + 2, *inliers, H);
    return CVO_OK;
}

// Not in the reference: the terms function_inner_product adds up, kept per point (include/cvo_hip.h, "per-point support")
int cvo_point_support(cvo_handle h, int slot_a, const float* tran_a, int slot_b, float* sum_a, int* count_a, int cap_a, float* sum_b, int* count_b, int cap_b) {
    if (!h) return fail(CVO_ERR_INVALID, "null argument");
    if (!sum_a != !count_a || !sum_b != !count_b) return fail(CVO_ERR_INVALID, "point support: a direction needs its sum and its count array");
    if (!sum_a && !sum_b) return fail(CVO_ERR_INVALID, "point support: no output array");
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "point support: empty cloud slot");
    if ((sum_a && cap_a < a->n) || (sum_b && cap_b < b->n)) return fail(CVO_ERR_INVALID, "point support: an output array is shorter than its cloud");
    const Engine::SupportReq rq[1] = {{a, tran_a, b, h->ell, -1, false, {sum_a, count_a, sum_b, count_b}}};
    return h->eng.point_sides(rq, 1, h->eng.stream, true);
}

namespace {
int stage_clouds(cvo_handle h, const float* xyz_a, const float* feat_a, int n_a, const float* xyz_b, const float* feat_b, int n_b) {
    if (n_a <= 0 || n_b <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "empty cloud");
    int rc = h->eng.upload(h->scratch_a, xyz_a, feat_a, n_a); if (rc) return rc;
    return h->eng.upload(h->scratch_b, xyz_b, feat_b, n_b);
}
}  // namespace
int cvo_function_inner_product_clouds(cvo_handle h, const float* xyz_a, const float* feat_a, int n_a, const float* xyz_b, const float* feat_b, int n_b,
                                      cvo_inn_p* out) {
    if (!h || !out) return fail(CVO_ERR_INVALID, "null argument");
    int rc = stage_clouds(h, xyz_a, feat_a, n_a, xyz_b, feat_b, n_b); if (rc) return rc;
    double r[1][24];
    const Engine::ScoreReq rq[1] = {{&h->scratch_a, nullptr, &h->scratch_b, false, h->ell}};
    rc = h->eng.score_many(rq, 1, r); if (rc) return rc;
    finish_inn_p(r[0], out);
    return CVO_OK;
}
int cvo_se3_hessian_clouds(cvo_handle h, const float* xyz_a, const float* feat_a, int n_a, const float* xyz_b, const float* feat_b, int n_b,
                           double H[36], int* inliers) {
    if (!h || !H || !inliers) return fail(CVO_ERR_INVALID, "null argument");
    int rc = stage_clouds(h, xyz_a, feat_a, n_a, xyz_b, feat_b, n_b); if (rc) return rc;
    double r[1][24];
    const Engine::ScoreReq rq[1] = {{&h->scratch_a, nullptr, &h->scratch_b, true, h->ell}};
    rc = h->eng.score_many(rq, 1, r); if (rc) return rc;
    *inliers += (int)r[0][1];                                        // cvo.cpp:708
    finish_hessian(r[0] + 2, *inliers, H);
    return CVO_OK;
}

// The whole score block of the tracker is one launch (the reference runs 4 KD-tree builds + 5 sweeps, cvo.cpp:489-500).
int cvo_compute_innerproduct(cvo_handle h, cvo_inn_p* inn_pre, cvo_inn_p* inn_post, double post_hessian[36], const float tran[12],
                             int* inliers, cvo_inn_p* inn_fixed_pcd, cvo_inn_p* inn_moving_pcd, float* cos_angle) {
    if (!h || !inn_pre || !inn_post || !post_hessian || !tran || !inliers || !inn_fixed_pcd || !inn_moving_pcd || !cos_angle)
        return fail(CVO_ERR_INVALID, "null argument");
    Cloud* fx = slot_cloud(h, CVO_SLOT_FIXED); Cloud* mv = slot_cloud(h, CVO_SLOT_MOVING);
    if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "function_inner_product: empty cloud slot");
    const Engine::ScoreReq rq[5] = {{mv, nullptr, fx, false, h->ell},        // cvo.cpp:489
                                    {mv, tran, fx, false, h->ell},           // cvo.cpp:491
                                    {fx, nullptr, fx, false, h->ell},        // cvo.cpp:496
                                    {mv, nullptr, mv, false, h->ell},        // cvo.cpp:497
                                    {mv, tran, fx, true, h->ell}};           // cvo.cpp:500
    double r[5][24];
    int rc;
    if (h->eng.launched && std::memcmp(h->transform.m, tran, sizeof(float) * 12) == 0) h->asked_after_align = true;   // the tracker's pattern: the next alignment starts this block itself (mode 2)
    if (h->queued_valid && h->eng.score_pending == 5) {
        // queued behind the align kernel for the alignment's own transform and ell (do_align): for exactly that question the answers are on their way or there
        const bool same = h->queued_fixed == fx && h->queued_moving == mv && h->queued_ell == h->ell && std::memcmp(h->queued_tran, tran, sizeof(h->queued_tran)) == 0;
        h->queued_valid = false;
        rc = h->eng.score_collect(5, r); if (rc) return rc;          // (collected either way: the pinned block is free again)
        if (!same) { rc = h->eng.score_many(rq, 5, r); if (rc) return rc; } else ++h->queued_hits;
    } else if (h->tail_valid && h->tail_fixed == fx && h->tail_moving == mv && h->tail_ell == h->ell && std::memcmp(h->tail_tran, tran, sizeof(h->tail_tran)) == 0) {
        // answered by the align launch itself; what its workgroups could not answer (PairDesc::score_out[23]) goes to the score kernel now
        std::memcpy(r, h->tail_r, sizeof(r));
        static const int bit_of[5] = {TAIL_PRE, TAIL_POST, TAIL_FIXED, TAIL_MOVING, TAIL_HESSIAN};
        const int mask = (int)r[0][23];
        Engine::ScoreReq miss[5]; int where[5], nmiss = 0;
        for (int q = 0; q < 5; ++q) if (!(mask & bit_of[q])) { miss[nmiss] = rq[q]; where[nmiss++] = q; }
        if (nmiss) {
            double extra[5][24];
            rc = h->eng.score_many(miss, nmiss, extra); if (rc) return rc;
            for (int k = 0; k < nmiss; ++k) std::memcpy(r[where[k]], extra[k], sizeof(double) * 24);
        }
    } else {
        rc = h->eng.score_many(rq, 5, r); if (rc) return rc;
    }
    finish_inn_p(r[0], inn_pre); finish_inn_p(r[1], inn_post); finish_inn_p(r[2], inn_fixed_pcd); finish_inn_p(r[3], inn_moving_pcd);
    *cos_angle = inn_post->value / (sqrtf(inn_fixed_pcd->value) * sqrtf(inn_moving_pcd->value));                  // cvo.cpp:498
    *inliers += (int)r[4][1];                                        // cvo.cpp:708
    finish_hessian(r[4] + 2, *inliers, post_hessian);
    return CVO_OK;
}

int cvo_compute_innerproduct_lc(cvo_handle h, cvo_inn_p* inn_prior, cvo_inn_p* inn_lc_prior, cvo_inn_p* inn_lc_pre, cvo_inn_p* inn_lc_post,
                                double post_hessian[36], const float prior_tran[12], const float lc_prior_tran[12],
                                const float lc_prior_tran_2[12], const float lc_tran[12], int* inliers_svd, int* inliers_pnpransac,
                                cvo_inn_p* inn_fixed_pcd, cvo_inn_p* inn_moving_pcd, float* cos_angle) {
    if (!h || !inn_prior || !inn_lc_prior || !inn_lc_pre || !inn_lc_post || !post_hessian || !prior_tran || !lc_prior_tran ||
        !lc_prior_tran_2 || !lc_tran || !inliers_svd || !inliers_pnpransac || !inn_fixed_pcd || !inn_moving_pcd || !cos_angle)
        return fail(CVO_ERR_INVALID, "null argument");
    Cloud* fx = slot_cloud(h, CVO_SLOT_FIXED); Cloud* mv = slot_cloud(h, CVO_SLOT_MOVING);
    if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "function_inner_product: empty cloud slot");
    const Engine::ScoreReq rq[8] = {{mv, prior_tran, fx, false, h->ell},     // cvo.cpp:539
                                    {mv, lc_prior_tran, fx, false, h->ell},  // cvo.cpp:541
                                    {mv, nullptr, fx, false, h->ell},        // cvo.cpp:543
                                    {mv, lc_tran, fx, false, h->ell},        // cvo.cpp:545
                                    {fx, nullptr, fx, false, h->ell},        // cvo.cpp:550
                                    {mv, nullptr, mv, false, h->ell},        // cvo.cpp:551
                                    {mv, lc_tran, fx, true, h->ell},         // cvo.cpp:555
                                    {mv, lc_prior_tran_2, fx, true, h->ell}};   // cvo.cpp:558
    double r[8][24];
    int rc = h->eng.score_many(rq, 8, r); if (rc) return rc;
    finish_inn_p(r[0], inn_prior); finish_inn_p(r[1], inn_lc_prior); finish_inn_p(r[2], inn_lc_pre); finish_inn_p(r[3], inn_lc_post);
    finish_inn_p(r[4], inn_fixed_pcd); finish_inn_p(r[5], inn_moving_pcd);
    *cos_angle = inn_lc_post->value / (sqrtf(inn_fixed_pcd->value) * sqrtf(inn_moving_pcd->value));                       // cvo.cpp:552
    *inliers_svd = (int)r[6][1];                                                                                          // cvo.cpp:554-555
    finish_hessian(r[6] + 2, *inliers_svd, post_hessian);
    *inliers_pnpransac = (int)r[7][1];                                                                                    // cvo.cpp:557-558 (only the inlier count is used)
    return CVO_OK;
}

int cvo_update_fixed_pcd(cvo_handle h) { if (!h) return fail(CVO_ERR_INVALID, "null handle"); slots_changed(h); h->fixed = std::move(h->moving); return CVO_OK; }
int cvo_update_previous_pcd(cvo_handle h) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    slots_changed(h); h->previous = std::move(h->moving); h->pre_pc_init = true; return CVO_OK;
}
int cvo_reset_transform(cvo_handle h, const float odometry[12]) {
    if (!h || !odometry) return fail(CVO_ERR_INVALID, "null argument");
    std::memcpy(h->transform.m, odometry, sizeof(float) * 12); return CVO_OK;
}
int cvo_reset_keyframe(cvo_handle h, const float odometry[12]) {
    if (!h || !odometry) return fail(CVO_ERR_INVALID, "null argument");
    slots_changed(h);
    if (!h->pre_pc_init) { h->fixed = std::move(h->moving); }
    else { h->fixed = std::move(h->previous); cvo_update_previous_pcd(h); }
    return cvo_reset_transform(h, odometry);
}
int cvo_reset_initial(cvo_handle h, const float odometry[12], float init_inverse_out[12]) {
    if (!h || !odometry) return fail(CVO_ERR_INVALID, "null argument");
    float back[12];
    reset_initial_eval(h->transform.m, odometry, h->R, h->T, back);   // cvo.cpp:613-617 (cvo_math.hpp)
    if (init_inverse_out) std::memcpy(init_inverse_out, back, sizeof(back));
    return CVO_OK;
}

int cvo_get_fixed_and_moving_number(cvo_handle h, int* fixed_num, int* moving_num) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (fixed_num) *fixed_num = h->num_fixed;
    if (moving_num) *moving_num = h->num_moving;
    return CVO_OK;
}
int cvo_get_iteration_number(cvo_handle h, int* iteration) { if (!h || !iteration) return fail(CVO_ERR_INVALID, "null argument"); *iteration = h->iter; return CVO_OK; }
int cvo_get_A_nonzero(cvo_handle h, int* nonzero) { if (!h || !nonzero) return fail(CVO_ERR_INVALID, "null argument"); *nonzero = h->A_nonzero; return CVO_OK; }
int cvo_get_transform(cvo_handle h, float transform[12]) { if (!h || !transform) return fail(CVO_ERR_INVALID, "null argument"); std::memcpy(transform, h->transform.m, sizeof(float) * 12); return CVO_OK; }
int cvo_get_prev_accum_transform(cvo_handle h, float prev_transform[12], float accum_transform[12]) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (prev_transform) std::memcpy(prev_transform, h->prev_transform.m, sizeof(float) * 12);
    if (accum_transform) std::memcpy(accum_transform, h->accum_transform.m, sizeof(float) * 12);
    return CVO_OK;
}
int cvo_get_init(cvo_handle h, int* init) { if (!h || !init) return fail(CVO_ERR_INVALID, "null argument"); *init = h->init ? 1 : 0; return CVO_OK; }
int cvo_get_first_frame(cvo_handle h, int* first_frame) { if (!h || !first_frame) return fail(CVO_ERR_INVALID, "null argument"); *first_frame = h->first_frame ? 1 : 0; return CVO_OK; }
int cvo_set_first_frame(cvo_handle h, int first_frame) { if (!h) return fail(CVO_ERR_INVALID, "null handle"); h->first_frame = first_frame != 0; return CVO_OK; }
int cvo_get_state(cvo_handle h, float R[9], float T[3], float* ell) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (R) std::memcpy(R, h->R, sizeof(h->R));
    if (T) std::memcpy(T, h->T, sizeof(h->T));
    if (ell) *ell = h->ell;
    return CVO_OK;
}
int cvo_set_state(cvo_handle h, const float R[9], const float T[3], float ell) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (R) std::memcpy(h->R, R, sizeof(h->R));
    if (T) std::memcpy(h->T, T, sizeof(h->T));
    h->ell = ell;
    return CVO_OK;
}
int cvo_set_workgroups(cvo_handle h, int workgroups_per_pair) {
    if (!h || workgroups_per_pair < 0) return fail(CVO_ERR_INVALID, "bad argument");
    h->eng.wg_request = workgroups_per_pair; return CVO_OK;
}
int cvo_set_arith_mode(cvo_handle h, int flags) {
    if (!h) return fail(CVO_ERR_INVALID, "null handle");
    if (flags & ~CVO_ARITH_EIGEN337) return fail(CVO_ERR_INVALID, "unknown arithmetic mode bit");
    h->eng.arith = flags; return CVO_OK;
}
int cvo_get_arith_mode(cvo_handle h, int* flags) { if (!h || !flags) return fail(CVO_ERR_INVALID, "null argument"); *flags = h->eng.arith; return CVO_OK; }

// ------------------------------------------------------------------ batches
namespace {
int selftest(int device, int kind, int n, const float* in, int in_w, float* out, int out_w) {
    int rc = check_device(device, nullptr); if (rc) return rc;
    if (n <= 0 || !in || !out) return fail(CVO_ERR_INVALID, "bad self-test arguments");
    HIP_TRY(hipSetDevice(device));
    DevBuf din, dout;
    if ((rc = din.ensure(sizeof(float) * (size_t)n * in_w)) || (rc = dout.ensure(sizeof(float) * (size_t)n * out_w))) { din.release(); dout.release(); return rc; }
    hipError_t e = hipMemcpy(din.p, in, sizeof(float) * (size_t)n * in_w, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = kind == 6 ? launch_selftest_reset_initial(static_cast<const float*>(din.p), static_cast<float*>(dout.p), n, nullptr)
                                       : launch_selftest(kind, static_cast<const float*>(din.p), static_cast<float*>(dout.p), n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, sizeof(float) * (size_t)n * out_w, hipMemcpyDeviceToHost);
    din.release(); dout.release();
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("self-test: ") + hipGetErrorString(e));
    return CVO_OK;
}
}  // namespace
int cvo_adaptive_default_params(cvo_adaptive_params* p) {
    if (!p) return fail(CVO_ERR_INVALID, "null params");
    p->ell_init = 0.1; p->ell_min = 0.0391; p->ell_max = 0.15; p->dl_step = 0.3;
    p->sigma = 0.1; p->sp_thres = 8.315e-3; p->c = 7.0; p->d = 7.0; p->c_ell = 0.5; p->c_sigma = 1;
    p->max_iter = 2000; p->min_step = 2 * 1.0e-1; p->eps = 5 * 1.0e-5; p->eps_2 = 1.0e-5;
    return CVO_OK;
}
int cvo_adaptive_align(int device, const cvo_adaptive_params* p_in, const float* fixed_xyz, const float* fixed_feat, int n_fixed,
                       const float* moving_xyz, const float* moving_feat, int n_moving, float R_inout[9], float T_inout[3], float* ell_out,
                       float transform_out[12], int* iter, cvo_adaptive_row* trace, int trace_cap, int* trace_len) {
    if (trace_len) *trace_len = 0;
    if (!R_inout || !T_inout) return fail(CVO_ERR_INVALID, "null pose");
    if (n_fixed <= 0 || n_moving <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "adaptive align: empty cloud");
    cvo_adaptive_params ap; if (p_in) ap = *p_in; else cvo_adaptive_default_params(&ap);
    cvo_params bp; cvo_default_params(&bp);
    Engine eng;
    int rc = eng.init(device, bp); if (rc) return rc;
    struct Guard { Engine& e; ~Guard() { e.destroy(); } } guard{eng};
    Cloud fx, mv;
    if ((rc = eng.upload(fx, fixed_xyz, fixed_feat, n_fixed))) return rc;
    if ((rc = eng.upload(mv, moving_xyz, moving_feat, n_moving))) return rc;
    DevBuf d_y, d_state, d_trace, d_len, d_part;
    struct Bufs { DevBuf *a, *b, *c, *d, *e; ~Bufs() { a->release(); b->release(); c->release(); d->release(); e->release(); } } bufs{&d_y, &d_state, &d_trace, &d_len, &d_part};
    const bool want_trace = trace && trace_cap > 0;
    if ((rc = d_y.ensure(sizeof(float4) * (size_t)n_moving)) || (rc = d_state.ensure(sizeof(AdaptiveState))) ||
        (rc = d_trace.ensure(sizeof(AdaptiveRow) * (size_t)std::max(1, trace_cap))) || (rc = d_len.ensure(sizeof(int) * 4)) ||
        (rc = d_part.ensure(sizeof(double) * 16 * (size_t)adaptive_partial_records(n_fixed, n_moving)))) return rc;
    AdaptiveState st; std::memset(&st, 0, sizeof(st));
    std::memcpy(st.R, R_inout, sizeof(st.R)); std::memcpy(st.T, T_inout, sizeof(st.T));
    st.ell = ap.ell_init; st.ell_max = ap.ell_max; st.iter = iter ? *iter : 0; st.status = -1;
    HIP_TRY(hipMemcpyAsync(d_state.p, &st, sizeof(st), hipMemcpyHostToDevice, eng.stream));
    HIP_TRY(hipMemsetAsync(d_len.p, 0, sizeof(int) * 4, eng.stream));
    AdaptiveArgs A; std::memset(&A, 0, sizeof(A));
    A.fixed = fx.rec(); A.moving = mv.rec(); A.nf = n_fixed; A.nm = n_moving;
    A.ybuf = static_cast<float4*>(d_y.p); A.state = static_cast<AdaptiveState*>(d_state.p);
    A.trace = want_trace ? static_cast<AdaptiveRow*>(d_trace.p) : nullptr; A.trace_cap = want_trace ? trace_cap : 0; A.trace_len = static_cast<int*>(d_len.p);
    A.ell_min = ap.ell_min; A.dl_step = ap.dl_step;
    A.P.sigma = ap.sigma; A.P.sp_thres = ap.sp_thres; A.P.c = ap.c; A.P.d = ap.d; A.P.c_ell = ap.c_ell; A.P.c_sigma = ap.c_sigma;
    A.P.min_step = ap.min_step; A.P.eps = ap.eps; A.P.eps_2 = ap.eps_2; A.P.max_iter = ap.max_iter; A.P.skin = 0.f; A.P.skin_alpha = 0.f; A.P.alpha_gamma = 0.f; A.P.first_scale = 1.f; A.P.fuse_refine = 0; A.P.nt_min = 0; A.P.overlap_stop_test = 0; A.P.predict = 0.f; A.P.predict_steps = 0.f; A.P.resort = 0; A.P.adopt_kmax = 0; A.P.adopt_on = 0; A.P.adopt_inject = 0; A.P.adopt_dwell = 0; A.P.colocate = 0;
    A.partials = static_cast<double*>(d_part.p);
    // a few iterations are queued at a time (five small kernels each, the rows of the sweeps spread over the device); kernels queued behind a
    // stop return at once, and the host looks at the stop flag between the chunks
    if (ap.max_iter <= 0) { st.status = 0; st.stop = 1; HIP_TRY(hipMemcpy(d_state.p, &st, sizeof(st), hipMemcpyHostToDevice)); }
    for (int done = 0; done < std::max(ap.max_iter, 0);) {
        const int chunk = std::min(8, ap.max_iter - done);
        hipError_t e = launch_adaptive(A, chunk, eng.stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("adaptive kernel launch: ") + hipGetErrorString(e));
        int stop = 0;
        HIP_TRY(hipMemcpyAsync(&stop, &static_cast<AdaptiveState*>(d_state.p)->stop, sizeof(int), hipMemcpyDeviceToHost, eng.stream));
        HIP_TRY(hipStreamSynchronize(eng.stream));
        done += chunk;
        if (stop) break;
    }
    HIP_TRY(hipMemcpy(&st, d_state.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st.status != 0) return fail(CVO_ERR_HIP, "adaptive kernel did not complete");
    std::memcpy(R_inout, st.R, sizeof(st.R)); std::memcpy(T_inout, st.T, sizeof(st.T));
    if (ell_out) *ell_out = st.ell;
    if (transform_out) std::memcpy(transform_out, st.transform, sizeof(float) * 12);
    if (iter) *iter = st.iter;
    if (want_trace) {
        int n = 0; HIP_TRY(hipMemcpy(&n, d_len.p, sizeof(int), hipMemcpyDeviceToHost));
        n = std::min(n, trace_cap);
        if (n > 0) HIP_TRY(hipMemcpy(trace, d_trace.p, sizeof(AdaptiveRow) * (size_t)n, hipMemcpyDeviceToHost));
        if (trace_len) *trace_len = n;
    }
    return CVO_OK;
}

int cvo_selftest_cubic_step(int device, int n, const float* coef_minstep, float* step_out) { return selftest(device, 0, n, coef_minstep, 5, step_out, 1); }
int cvo_selftest_exp_sek3(int device, int n, const float* omega_v_dt, float* dR_dT_out) { return selftest(device, 1, n, omega_v_dt, 7, dR_dT_out, 12); }
int cvo_selftest_dist_se3(int device, int n, const float* dR_dT, float* dist_out) { return selftest(device, 2, n, dR_dT, 12, dist_out, 1); }
int cvo_selftest_libm(int device, int n, const float* x, float* out6) { return selftest(device, 3, n, x, 1, out6, 6); }
int cvo_selftest_cubic_step_f32eig(int device, int n, const float* coef_minstep, float* step_out) { return selftest(device, 4, n, coef_minstep, 5, step_out, 1); }
int cvo_selftest_dist_se3_f32logm(int device, int n, const float* dR_dT, float* dist_out) { return selftest(device, 5, n, dR_dT, 12, dist_out, 1); }
int cvo_selftest_reset_initial(int device, int n, const float* transform_odometry, float* out) { return selftest(device, 6, n, transform_odometry, 24, out, 24); }
int cvo_selftest_pair_values(int device, const cvo_params* params, float ell, int n, const float* y_g, float* a_out, float* d2_d2c_out) {
    int rc = check_device(device, nullptr); if (rc) return rc;
    if (n <= 0 || !y_g || !a_out || !(ell > 0.f)) return fail(CVO_ERR_INVALID, "bad self-test arguments");
    cvo_params p; if (params) p = *params; else cvo_default_params(&p);
    HIP_TRY(hipSetDevice(device));
    DevBuf din, dout, daux;
    if ((rc = din.ensure(sizeof(float) * (size_t)n * 8)) || (rc = dout.ensure(sizeof(float) * (size_t)n * 4)) || (rc = daux.ensure(sizeof(float) * (size_t)n * 2))) {
        din.release(); dout.release(); daux.release(); return rc;
    }
    hipError_t e = hipMemcpy(din.p, y_g, sizeof(float) * (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest_pairs(static_cast<const float*>(din.p), static_cast<float*>(dout.p), static_cast<float*>(daux.p), n, ell, to_dev(p), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(a_out, dout.p, sizeof(float) * (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && d2_d2c_out) e = hipMemcpy(d2_d2c_out, daux.p, sizeof(float) * (size_t)n * 2, hipMemcpyDeviceToHost);
    din.release(); dout.release(); daux.release();
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("self-test: ") + hipGetErrorString(e));
    return CVO_OK;
}
int cvo_selftest_voxel_slots(int device, int n, const float* xyz, float voxel, unsigned slots, int* valid_out, unsigned long long* key_out, unsigned* slot_out) {
    int rc = check_device(device, nullptr); if (rc) return rc;
    if (n <= 0 || !xyz || !valid_out || !key_out || !slot_out || !(voxel > 0.f) || !std::isfinite(voxel) || slots == 0u) return fail(CVO_ERR_INVALID, "bad self-test arguments");
    HIP_TRY(hipSetDevice(device));
    DevBuf din, dvalid, dkey, dslot;
    if ((rc = din.ensure(sizeof(float) * (size_t)n * 3)) || (rc = dvalid.ensure(sizeof(int) * (size_t)n)) || (rc = dkey.ensure(sizeof(unsigned long long) * (size_t)n)) ||
        (rc = dslot.ensure(sizeof(unsigned) * (size_t)n))) {
        din.release(); dvalid.release(); dkey.release(); dslot.release(); return rc;
    }
    hipError_t e = hipMemcpy(din.p, xyz, sizeof(float) * (size_t)n * 3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest_voxel_slots(static_cast<const float*>(din.p), n, voxel, slots, static_cast<int*>(dvalid.p), static_cast<unsigned long long*>(dkey.p),
                                                         static_cast<unsigned*>(dslot.p), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(valid_out, dvalid.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(key_out, dkey.p, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(slot_out, dslot.p, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost);
    din.release(); dvalid.release(); dkey.release(); dslot.release();
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("self-test: ") + hipGetErrorString(e));
    return CVO_OK;
}

namespace {
// The last launch's results taken in once it is over: listed slots that had no moving cloud get CVO_ERR_NOT_INITIALIZED (cvo.cpp:463-466),
// and every stream slot that was aligned carries what its alignment left behind, exactly as do_align takes it into a handle (a failed
// alignment leaves the object as it was).  A no-op unless the last launch listed stream slots.
int batch_settle(cvo_batch b) {
    if (b->settled) return CVO_OK;
    b->settled = true;
    int rc = b->eng.wait(); if (rc) return rc;
    PairState* r = static_cast<PairState*>(b->eng.h_states.p);      // (pinned host memory the kernel wrote)
    for (int i = 0; i < b->last_n; ++i) {
        if (b->last_not_run[i]) { r[i].status = CVO_ERR_NOT_INITIALIZED; continue; }
        if (!b->last_stream_pos[i] || r[i].status != CVO_OK) continue;
        StreamSlot& S = b->streams[b->last_slots[i]];
        std::memcpy(S.R, r[i].R, sizeof(S.R)); std::memcpy(S.T, r[i].T, sizeof(S.T));
        S.ell = r[i].ell; S.iter = r[i].iter;
        Aff prev; std::memcpy(prev.m, r[i].prev_transform, sizeof(prev.m));
        S.prev_transform = prev;                                     // cvo.cpp:815
        S.accum_transform = aff_mul(S.accum_transform, prev);        // cvo.cpp:816
        std::memcpy(S.transform.m, r[i].transform, sizeof(S.transform.m));   // update_tf, cvo.cpp:817
    }
    return CVO_OK;
}
// a fresh cvo::cvo in slot p (cvo.cpp:28-70): no clouds, R = I, T = 0, ell = params.ell, every transform I
void fresh_stream(cvo_batch b, int p) {
    StreamSlot& S = b->streams[p];
    S = StreamSlot();
    S.on = true;
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(S.R, I, sizeof(I)); S.T[0] = S.T[1] = S.T[2] = 0.f; S.ell = b->prm.ell;
    S.transform = S.prev_transform = S.accum_transform = aff_identity();
    for (Cloud* c : {b->fixed[p].get(), b->moving[p].get()})
        if (c) { c->n = 0; c->n_px = 0; c->boxes_valid = false; c->raw = nullptr; c->raw_feat = nullptr; c->cost_hint = 0.f; }
}
// A slot's cloud objects before they are written or emptied through the slot: one that other slots hold too is let go of (the pool keeps it)
void own_slot_clouds(cvo_batch b, int p) { for (std::shared_ptr<Cloud>* c : {&b->fixed[p], &b->moving[p]}) if (*c && (*c)->multi) c->reset(); }
void report_step_laps(const char* who); void stage_drop(cvo_batch b); void stage_drop_if_listed(cvo_batch b, int p); void stage_destroy(cvo_batch b); int stage_place(cvo_batch b, bool block);   // (the stage: below, behind the generator)
// what every set_* did to the single flag it had: each plain pair starts its next launch from init_states again.  Slots set here stop being streams.
void states_dirty(cvo_batch b) { std::fill(b->dirty.begin(), b->dirty.end(), (unsigned char)1); }
void end_stream(cvo_batch b, int p) { stage_drop_if_listed(b, p); if (b->streams[p].on) { b->streams[p] = StreamSlot(); fresh_state(b->init_states[p], b->prm.ell); } }
// A slot of the last launch got new clouds: answers held for them (score blocks computed from the slots' clouds) would be for others
void slot_clouds_changed(cvo_batch b, int p) {
    for (int i = 0; i < b->last_n && !b->clouds_changed; ++i) b->clouds_changed = b->last_slots[i] == p;
}
int check_last_clouds(cvo_batch b) {
    return b->clouds_changed ? fail(CVO_ERR_INVALID, "the clouds of a slot of the last launch have changed since (cvo_batch_advance_images / cvo_batch_reset_stream)") : CVO_OK;
}
// One persistent launch over the listed slots, position i = slots[i].  Plain pairs start from init_states when marked dirty, else from their
// device state; stream slots from the state they carry, like a handle's align(); a stream slot without a moving cloud takes a position that
// runs nothing (no moving cloud: the kernel leaves at once) and its entry reads CVO_ERR_NOT_INITIALIZED.  clean_all: every plain pair counts as
// started afterwards (cvo_batch_align_async, as the single flag was cleared), else only the listed ones.
int batch_launch(cvo_batch b, const int* slots, int n, hipStream_t stream, bool clean_all) {
    int rc = batch_settle(b); if (rc) return rc;
    std::vector<Engine::PairIn> pairs(n);
    std::vector<PairState> st(n);
    std::vector<unsigned char> up(n, 0), is_stream(n, 0), not_run(n, 0);
    bool any_stream = false;
    for (int i = 0; i < n; ++i) {
        const int p = slots[i];
        const StreamSlot& S = b->streams[p];
        pairs[i] = Engine::PairIn{b->fixed[p].get(), b->moving[p].get()};
        if (S.on) {
            any_stream = true; is_stream[i] = 1; up[i] = 1;
            carried_state(st[i], S.R, S.T, S.ell, S.iter, S.transform);
            if (!S.has_moving) { not_run[i] = 1; pairs[i].moving = nullptr; if (!S.init) pairs[i].fixed = nullptr; }
        } else {
            up[i] = b->dirty[p]; st[i] = b->init_states[p];
        }
    }
    // a seed queued on the object's stream (cvo_batch_seed_hypotheses_async) comes before a launch on a caller's stream: it writes the start states
    if (stream && stream != b->eng.stream && b->eng.hyp_call.queued) HIP_TRY(hipStreamWaitEvent(stream, b->eng.hyp_call.done, 0));
    rc = b->eng.launch(pairs, st.data(), false, stream, false, 0, slots, up.data());
    if (rc) return rc;
    if (clean_all) std::fill(b->dirty.begin(), b->dirty.end(), (unsigned char)0);   // device states now evolve launch to launch (warm start) until reset
    else for (int i = 0; i < n; ++i) if (!is_stream[i]) b->dirty[slots[i]] = 0;
    b->last_n = n;
    b->last_slots.assign(slots, slots + n); b->last_stream_pos = is_stream; b->last_not_run = not_run;
    b->settled = !any_stream; b->clouds_changed = false;
    for (int i = 0; i < n; ++i) {
        if (!not_run[i]) continue;
        const hipError_t e = launch_fill_records(static_cast<float*>(b->eng.d_records.p), i, i + 1, CVO_ERR_NOT_INITIALIZED, b->eng.last_stream);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("record fill kernel launch: ") + hipGetErrorString(e));
    }
    return CVO_OK;
}
}  // namespace

// dealt: the object's stream may take the second queue class (Engine::make_stream) -- the batch objects a caller makes; the two inside a tracker
// object stay normal, their launches go on a stream that holds other work of the step (queue_behind)
static int batch_create(const cvo_params* p, int device, int max_pairs, cvo_batch* out, bool dealt) {
    if (!out || max_pairs <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    *out = nullptr;
    std::unique_ptr<cvo_batch_s> b(new cvo_batch_s());
    if (p) b->prm = *p; else cvo_default_params(&b->prm);
    int rc = b->eng.init(device, b->prm, dealt); if (rc) { b->eng.destroy(); return rc; }
    b->max_pairs = max_pairs;
    b->eng.defer_pack = true;                                       // hand-overs are packed by the next align launch (Engine::upload_many)
    b->eng.rec_hint = max_pairs + 1;                                // room for the padding record of an uneven shard (cvo_shard_range)
    b->eng.coop_first_scale = 1.75f;                                // few pairs on many workgroups each = loop-closure candidates: wider first lists (launch_impl)
    b->fixed.resize(max_pairs); b->moving.resize(max_pairs);
    b->init_states.resize(max_pairs);
    for (auto& s : b->init_states) fresh_state(s, b->prm.ell);
    b->dirty.assign(max_pairs, 1);
    b->streams.resize(max_pairs);
    b->eng.state_slots = max_pairs;                                 // a device state per slot, whichever positions its launches give it
    *out = b.release();
    return CVO_OK;
}
int cvo_batch_create(const cvo_params* p, int device, int max_pairs, cvo_batch* out) { return batch_create(p, device, max_pairs, out, true); }
int cvo_batch_destroy(cvo_batch b) {
    if (!b) return CVO_OK;
    (void)hipSetDevice(b->eng.device);
    stage_destroy(b);                                               // (drains the stage stream first)
    if (b->eng.stream) (void)hipStreamSynchronize(b->eng.stream);
    b->fixed.clear(); b->moving.clear(); b->pool.clear();
    b->img.release(); b->cin.release();
    report_step_laps("batch");
    b->eng.destroy();
    delete b;
    return CVO_OK;
}
int cvo_batch_set_pair(cvo_batch b, int p, const float* fixed_xyz, const float* fixed_feat, int n_fixed,
                       const float* moving_xyz, const float* moving_feat, int n_moving) {
    if (!b || p < 0 || p >= b->max_pairs) return fail(CVO_ERR_INVALID, "bad pair index");
    int rc = batch_settle(b); if (rc) return rc;
    own_slot_clouds(b, p);
    if (!b->fixed[p]) b->fixed[p].reset(new Cloud());
    if (!b->moving[p]) b->moving[p].reset(new Cloud());
    end_stream(b, p);
    rc = b->eng.upload(*b->fixed[p], fixed_xyz, fixed_feat, n_fixed); if (rc) return rc;
    rc = b->eng.upload(*b->moving[p], moving_xyz, moving_feat, n_moving); if (rc) return rc;
    fresh_state(b->init_states[p], b->prm.ell);
    states_dirty(b);
    return CVO_OK;
}
int cvo_batch_set_pairs(cvo_batch b, int first, int count, const float* const* fixed_xyz, const float* const* fixed_feat, const int* n_fixed,
                        const float* const* moving_xyz, const float* const* moving_feat, const int* n_moving) {
    if (!b || first < 0 || count <= 0 || first + count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad pair range");
    if (!fixed_xyz || !fixed_feat || !n_fixed || !moving_xyz || !moving_feat || !n_moving) return fail(CVO_ERR_INVALID, "null argument");
    int rc = batch_settle(b); if (rc) return rc;
    std::vector<Engine::UploadItem> items; items.reserve(2 * (size_t)count);
    for (int k = 0; k < count; ++k) {
        const int p = first + k;
        end_stream(b, p);
        own_slot_clouds(b, p);
        if (!b->fixed[p]) b->fixed[p].reset(new Cloud());
        if (!b->moving[p]) b->moving[p].reset(new Cloud());
        items.push_back(Engine::UploadItem{b->fixed[p].get(), fixed_xyz[k], fixed_feat[k], n_fixed[k]});
        items.push_back(Engine::UploadItem{b->moving[p].get(), moving_xyz[k], moving_feat[k], n_moving[k]});
    }
    rc = b->eng.upload_many(items.data(), (int)items.size()); if (rc) return rc;
    for (int k = 0; k < count; ++k) fresh_state(b->init_states[first + k], b->prm.ell);
    states_dirty(b);
    return CVO_OK;
}

// ---- clouds from RGB-D images: every image generated once by the batched generator (cvo_pcd_kernels.hip, a fixed list of launches over all
// images, makeMaps decided on the device), ONE host sync for the point counts, then each destination cloud copied from its image's slot
namespace {
// CVO_HIP_STEP_LAPS=1: host timers around the stages of a K-stream step, added up and printed (stderr, ms per step) when the object is destroyed.
// A measuring mode: it waits for each host-to-device copy where it is queued, so that the copy's time is its own lap and not the generator's.
struct StepLaps {
    enum { COPY, H2D, GENERATE, SCATTER, LAUNCH, WAIT, COMMIT, STAGE, CONSUME, INGEST, N };
    bool on = false; double ms[N] = {}; long steps = 0;
};
StepLaps* step_laps() {
    static StepLaps L = [] { StepLaps l; const char* e = std::getenv("CVO_HIP_STEP_LAPS"); l.on = e && std::atoi(e) != 0; return l; }();
    return &L;
}
struct Lap {
    int k; std::chrono::steady_clock::time_point t0;
    explicit Lap(int k_) : k(k_) { if (step_laps()->on) t0 = std::chrono::steady_clock::now(); }
    ~Lap() { if (step_laps()->on) step_laps()->ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
void report_step_laps(const char* who) {
    StepLaps& L = *step_laps();
    if (!L.on || L.steps <= 0) return;
    static const char* name[StepLaps::N] = {"host_copy", "h2d_copy", "generate_to_sync", "scatter", "launches", "wait", "commit", "stage_call", "consume_call", "ingest"};
    std::fprintf(stderr, "[cvo_hip] %s step laps, ms per step over %ld steps:", who, L.steps);
    for (int q = 0; q < StepLaps::N; ++q) std::fprintf(stderr, " %s %.3f", name[q], L.ms[q] / (double)L.steps);
    std::fprintf(stderr, "\n");
    L = StepLaps(); L.on = true;
}
// The images of a call: host images (bgr8 / depth16, one pointer per image) or caller-owned device images (dev, checked by check_device_images)
// with the stream their writer ran on (image_stream; null = the caller has synchronised it).
struct ImageSrc {
    const unsigned char* const* bgr8 = nullptr; const unsigned short* const* depth16 = nullptr;
    const cvo_device_image* dev = nullptr; hipStream_t image_stream = nullptr;
    static ImageSrc host(const unsigned char* const* bgr8, const unsigned short* const* depth16) { ImageSrc s; s.bgr8 = bgr8; s.depth16 = depth16; return s; }
    static ImageSrc device(const cvo_device_image* images, void* image_stream) { ImageSrc s; s.dev = images; s.image_stream = static_cast<hipStream_t>(image_stream); return s; }
};
// The fill of the stacks from device images: ONE ingest launch on s, which is always a stream of the library's own -- a caller's stream may share
// the hardware queue of a persistent align launch and would not start before that launch ends.  With an image_stream: s waits for what is queued
// there by an event, and the image_stream waits for the ingest by a second one (no host wait); without: the host waits for the ingest alone.
int ingest_enqueue(BatchImages& S, hipStream_t s, int N, const ImageSrc& src, int w, int h) {
    int rc;
    if ((rc = S.h_ingest.ensure(sizeof(PcdIngestDesc) * (size_t)S.n_cap))) return rc;
    if (!S.ev_in) HIP_TRY(hipEventCreateWithFlags(&S.ev_in, hipEventDisableTiming));
    if (!S.ev_out) HIP_TRY(hipEventCreateWithFlags(&S.ev_out, hipEventDisableTiming));
    PcdIngestDesc* d = static_cast<PcdIngestDesc*>(S.h_ingest.p);
    for (int k = 0; k < N; ++k) {
        const cvo_device_image& im = src.dev[k];
        d[k].bgr = static_cast<const uint8_t*>(im.bgr8); d[k].depth = static_cast<const uint8_t*>(im.depth16);
        d[k].bgr_pitch = im.bgr_pitch ? im.bgr_pitch : (long long)w * im.pixel_bytes;
        d[k].depth_pitch = im.depth_pitch ? im.depth_pitch : 2ll * w;
        d[k].pixel_bytes = im.pixel_bytes; d[k].swap_rb = im.swap_rb;
        d[k].bgr_dwords = ((reinterpret_cast<uintptr_t>(im.bgr8) | (uintptr_t)d[k].bgr_pitch) & 3u) == 0;
        d[k].depth_dwords = ((reinterpret_cast<uintptr_t>(im.depth16) | (uintptr_t)d[k].depth_pitch) & 3u) == 0;
    }
    if (src.image_stream) {
        HIP_TRY(hipEventRecord(S.ev_in, src.image_stream));
        HIP_TRY(hipStreamWaitEvent(s, S.ev_in, 0));
    }
    const hipError_t e = pcd_launch_ingest(d, (uint8_t*)S.bgr.p, (uint8_t*)S.depth.p, w, h, N, s);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd ingest kernel launch: ") + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(S.ev_out, s));
    Lap lap(StepLaps::INGEST);
    if (src.image_stream) HIP_TRY(hipStreamWaitEvent(src.image_stream, S.ev_out, 0));
    else HIP_TRY(hipEventSynchronize(S.ev_out));
    if (step_laps()->on) HIP_TRY(hipStreamSynchronize(s));
    return CVO_OK;
}
// N images (all w x h) queued for generation on stream s into the images' slots of S.cloud / S.px: the stacks filled, the generator's fixed list
// of launches, the read-back of the records into S.h_rec.  The fill: host images are copied into S's pinned stage (by `copy_parts` threads of
// the copy pool) and from there to the device, the colour images first so that the kernels that need nothing else run while the host stages
// the depth images; device images are gathered by the ingest launch (no pinned image stage, no copy threads).  Waits for nothing but a growing
// scratch (and a device call without image_stream for its ingest); the caller's images are free when it returns, device images given with an
// image_stream for work queued on that stream.  cam: one camera for all, or cam_table (host, N cameras): a camera per image.
int generate_enqueue(Engine& E, BatchImages& S, hipStream_t s, int N, const ImageSrc& src, int width, int height,
                     const cvo_camera* cam, const cvo_camera* cam_table, int copy_parts) {
    const unsigned char* const* bgr8 = src.bgr8; const unsigned short* const* depth16 = src.depth16;
    const int w = width, h = height, num_want = S.num_want;
    const size_t n = (size_t)w * h, n1 = (size_t)(w / 2) * (h / 2), n2 = (size_t)(w / 4) * (h / 4), nths = (size_t)(w / 32) * (h / 32) + 100;
    const int nt = pcd_tiles(w, h), cap = PCD_CLOUD_CAP;
    const bool laps = step_laps()->on;
    int rc;
    if (N > S.n_cap || w != S.w || h != S.h) {
        HIP_TRY(hipStreamSynchronize(s));                              // the previous call's copies out of the slots may still read them
        const size_t m = (size_t)std::max(N, S.n_cap);
        if ((rc = S.bgr.ensure(3 * n * m)) || (rc = S.depth.ensure(2 * n * m)) || (rc = S.map.ensure(n * m))) return rc;
        for (DevBuf* x : {&S.I0, &S.dx0, &S.dy0, &S.abs0}) if ((rc = x->ensure(sizeof(float) * n * m))) return rc;
        for (DevBuf* x : {&S.I1, &S.abs1}) if ((rc = x->ensure(sizeof(float) * n1 * m))) return rc;
        for (DevBuf* x : {&S.I2, &S.abs2}) if ((rc = x->ensure(sizeof(float) * n2 * m))) return rc;
        for (DevBuf* x : {&S.ths, &S.thsS}) if ((rc = x->ensure(sizeof(float) * nths * m))) return rc;
        if ((rc = S.tiles.ensure(sizeof(int) * 3 * (size_t)nt * m)) || (rc = S.rec.ensure(sizeof(PcdImgRec) * m))) return rc;
        if ((rc = S.cloud.ensure(sizeof(float) * REC * (size_t)cap * m)) || (rc = S.px.ensure(sizeof(uint16_t) * 2 * (size_t)cap * m))) return rc;
        if ((rc = S.h_rec.ensure(sizeof(PcdImgRec) * m))) return rc;
        if (w != S.w || h != S.h) {                                   // the byte pattern only depends on w*h: made once per size, shared by every image
            if ((rc = S.pattern.ensure(n))) return rc;
            std::vector<unsigned char> pat(n);
            Engine::rand_pattern(3141592u, pat.data(), n);
            HIP_TRY(hipMemcpy(S.pattern.p, pat.data(), n, hipMemcpyHostToDevice));
        }
        S.n_cap = (int)m; S.w = w; S.h = h;
    }
    if (cam_table && ((rc = S.cams.ensure(sizeof(cvo_camera) * (size_t)S.n_cap)) || (rc = S.h_cams.ensure(sizeof(cvo_camera) * (size_t)S.n_cap)))) return rc;
    if (!src.dev && (rc = S.stage.ensure(5 * n * (size_t)S.n_cap))) return rc;
    unsigned char* st = static_cast<unsigned char*>(S.stage.p);
    // image k of `src` (bytes each) to dst + bytes * k, the images dealt to the copy threads in runs
    auto copy_images = [&](unsigned char* dst, const void* const* src, size_t bytes) {
        Lap lap(StepLaps::COPY);
        const int parts = std::max(1, std::min(copy_parts, N));
        CopyPool::get().run(parts, [&](int q) { for (int k = (int)((long long)N * q / parts); k < (int)((long long)N * (q + 1) / parts); ++k) std::memcpy(dst + bytes * k, src[k], bytes); });
    };
    // the colour images first: their copy and the pyramid / threshold / select kernels (which need nothing else) run while the host stages the depth images
    if (src.dev) {
        if ((rc = ingest_enqueue(S, s, N, src, w, h))) return rc;
    } else {
        copy_images(st, reinterpret_cast<const void* const*>(bgr8), 3 * n);
        HIP_TRY(hipMemcpyAsync(S.bgr.p, st, 3 * n * N, hipMemcpyHostToDevice, s));
        if (laps) { Lap lap(StepLaps::H2D); HIP_TRY(hipStreamSynchronize(s)); }
    }
    HIP_TRY(hipMemsetAsync(S.ths.p, 0, sizeof(float) * nths * N, s));
    HIP_TRY(hipMemsetAsync(S.thsS.p, 0, sizeof(float) * nths * N, s));
    HIP_TRY(hipMemsetAsync(S.map.p, 0, n * N, s));
    HIP_TRY(hipMemsetAsync(S.rec.p, 0, sizeof(PcdImgRec) * N, s));
    float* abs0 = (float*)S.abs0.p; float* abs1 = (float*)S.abs1.p; float* abs2 = (float*)S.abs2.p; PcdImgRec* rec = (PcdImgRec*)S.rec.p;
    hipError_t e = pcd_launch_pyramid((const uint8_t*)S.bgr.p, w, h, (float*)S.I0.p, (float*)S.I1.p, (float*)S.I2.p, (float*)S.dx0.p, (float*)S.dy0.p, abs0, abs1, abs2, N, s);
    if (e == hipSuccess) e = pcd_launch_thresholds(abs0, w, h, (float*)S.ths.p, (float*)S.thsS.p, N, s);
    if (e == hipSuccess) e = pcd_launch_select_batch(abs0, abs1, abs2, (const float*)S.thsS.p, w, h, (uint8_t*)S.map.p, rec, N, num_want, s);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd kernels: ") + hipGetErrorString(e));
    if (!src.dev) {
        unsigned char* sd = st + 3 * n * N;
        copy_images(sd, reinterpret_cast<const void* const*>(depth16), 2 * n);
        if (laps) { Lap lap(StepLaps::GENERATE); HIP_TRY(hipStreamSynchronize(s)); }   // (the kernels queued so far: not part of the depth copy's lap)
        HIP_TRY(hipMemcpyAsync(S.depth.p, sd, 2 * n * N, hipMemcpyHostToDevice, s));
        if (laps) { Lap lap(StepLaps::H2D); HIP_TRY(hipStreamSynchronize(s)); }
    }
    const cvo_camera& c0 = cam ? *cam : cam_table[0];
    const float camv[5] = {c0.scaling_factor, c0.fx, c0.fy, c0.cx, c0.cy};
    if (cam_table) {
        std::memcpy(S.h_cams.p, cam_table, sizeof(cvo_camera) * (size_t)N);
        HIP_TRY(hipMemcpyAsync(S.cams.p, S.h_cams.p, sizeof(cvo_camera) * (size_t)N, hipMemcpyHostToDevice, s));
    }
    e = pcd_launch_subsample_batch((uint8_t*)S.map.p, (const uint8_t*)S.pattern.p, rec, num_want, (const uint16_t*)S.depth.p, w, h, (int*)S.tiles.p, N, s);
    if (e == hipSuccess) e = pcd_launch_cloud_batch((const uint8_t*)S.map.p, (const uint16_t*)S.depth.p, (const uint8_t*)S.bgr.p, (const float*)S.dx0.p, (const float*)S.dy0.p,
                                                    w, h, camv, cam_table ? (const float*)S.cams.p : nullptr, (const int*)S.tiles.p, rec, cap, (float*)S.cloud.p,
                                                    (uint16_t*)S.px.p, N, s);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd kernels: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(S.h_rec.p, S.rec.p, sizeof(PcdImgRec) * N, hipMemcpyDeviceToHost, s));
    return CVO_OK;
}
int check_cloud_caps(const PcdImgRec* R, int N) {
    for (int k = 0; k < N; ++k)
        if (R[k].npts > PCD_CLOUD_CAP) return fail(CVO_ERR_INVALID, "image " + std::to_string(k) + ": more than 65535 points per cloud is not supported (16-bit column indices)");
    return CVO_OK;
}
// The clouds of N images (all w x h) into the images' slots of b->img.cloud / px; *recs: their records on the host.  Nothing of the batch's pairs changes.
int batch_generate(cvo_batch b, int N, const ImageSrc& src, int width, int height, const cvo_camera* cam,
                   const cvo_camera* cam_table, const PcdImgRec** recs) {
    Engine& E = b->eng; BatchImages& S = b->img;
    HIP_TRY(hipSetDevice(E.device));
    hipStream_t s = E.stream;
    {
        // every return from here on leaves nothing of this call in flight: the next call overwrites the pinned stage the copies read from
        struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};
        int rc = generate_enqueue(E, S, s, N, src, width, height, cam, cam_table, 1); if (rc) return rc;
        Lap lap(StepLaps::GENERATE);
        (void)hipStreamSynchronize(s);
    }                                                                 // (the one sync)
    HIP_TRY(hipStreamSynchronize(s));                                 // (reports an error of the queued work; nothing left to wait for)
    const PcdImgRec* R = static_cast<const PcdImgRec*>(S.h_rec.p);
    int rc = check_cloud_caps(R, N); if (rc) return rc;
    *recs = R;
    return CVO_OK;
}
// clouds dst[j] <- image img[j]'s cloud of the last batch_generate (the scatter kernel, up to PCD_SCATTER_MAX clouds per launch); buffers are made first
int batch_scatter(cvo_batch b, const std::vector<Cloud*>& dst, const std::vector<int>& img, const PcdImgRec* R) {
    Engine& E = b->eng; BatchImages& S = b->img;
    const hipStream_t s = E.stream; const int cap = PCD_CLOUD_CAP;
    int rc;
    // (a launch on a caller's stream may still read the clouds they had)
    if (E.launched && E.last_stream && E.last_stream != s) HIP_TRY(hipStreamSynchronize(E.last_stream));
    for (size_t j = 0; j < dst.size(); ++j) {
        const int np = R[img[j]].npts;
        if (np > 0 && ((rc = dst[j]->buf.ensure((size_t)np * REC * sizeof(float))) || (rc = dst[j]->px.ensure((size_t)np * 2 * sizeof(uint16_t))))) return rc;
    }
    PcdScatter sc; std::memset(&sc, 0, sizeof(sc));
    sc.src = (const float*)S.cloud.p; sc.src_px = (const uint16_t*)S.px.p; sc.rec = (const PcdImgRec*)S.rec.p; sc.cap = cap;
    int n_max = 0;
    auto flush = [&]() -> int {
        const hipError_t e = pcd_launch_scatter(sc, n_max, s);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd scatter: ") + hipGetErrorString(e));
        sc.n = 0; n_max = 0; return CVO_OK;
    };
    for (size_t j = 0; j < dst.size(); ++j) {
        Cloud& c = *dst[j];
        const PcdImgRec& r = R[img[j]];
        c.n = r.npts; c.n_px = r.npts; c.boxes_valid = false; c.raw = nullptr; c.raw_feat = nullptr;   // (a hand-over not packed yet is dropped)
        c.cost_hint = r.cost_n > 0 ? (float)(r.cost / r.cost_n) : 0.f;
        if (c.n <= 0) continue;
        sc.img[sc.n] = img[j]; sc.dst[sc.n] = c.rec(); sc.dst_px[sc.n] = (uint16_t*)c.px.p; ++sc.n; n_max = std::max(n_max, c.n);
        if (sc.n == PCD_SCATTER_MAX && (rc = flush())) return rc;
    }
    if (sc.n > 0 && (rc = flush())) return rc;
    E.uploads_pending = true;                                         // (a launch on another stream waits for the copies: settle_uploads)
    return CVO_OK;
}
bool image_size_ok(int width, int height) { return width >= 64 && height >= 64 && (size_t)width * height <= (size_t)1 << 26; }
// One plane of a device image: rows of row_bytes bytes, `pitch` apart (resolved), `height` of them from ptr.  The device must be able to read
// every byte: device memory of `device` (the rows inside the allocation), managed memory, or pinned / registered host memory.  Anything else --
// pageable host memory, another device's memory -- is refused here, it must never reach a kernel.
int check_device_plane(int device, const void* ptr, long long pitch, long long row_bytes, int height, const std::string& what, const char* thing = "image") {
    hipPointerAttribute_t at; std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(CVO_ERR_INVALID, what + ": not a pointer the device can read (" + hipGetErrorString(e) + ")"); }
    if (at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost) return CVO_OK;
    if (at.type != hipMemoryTypeDevice) return fail(CVO_ERR_INVALID, what + ": unregistered host memory, the device cannot read it");
    if (at.device != device) return fail(CVO_ERR_INVALID, what + ": memory of device " + std::to_string(at.device) + ", the object runs on device " + std::to_string(device));
    hipDeviceptr_t base = nullptr; size_t size = 0;
    const hipError_t er = hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr));
    if (er != hipSuccess) { (void)hipGetLastError(); return fail(CVO_ERR_INVALID, what + ": no allocation found around the pointer (" + hipGetErrorString(er) + ")"); }
    const unsigned long long lo = reinterpret_cast<uintptr_t>(ptr), a0 = reinterpret_cast<uintptr_t>(base);
    const unsigned long long need = (unsigned long long)(height - 1) * (unsigned long long)pitch + (unsigned long long)row_bytes;
    if (lo < a0 || lo - a0 > size || need > size - (lo - a0)) return fail(CVO_ERR_INVALID, what + ": the " + thing + " ends outside its allocation (" + std::to_string(need) + " bytes from the pointer)");
    return CVO_OK;
}
// What every device entry point checks first, before any stream changes and before anything is queued (cvo_check_device_images runs it alone).
int check_device_images(int device, int count, const cvo_device_image* images, int width, int height) {
    if (count <= 0 || count > 65535) return fail(CVO_ERR_INVALID, "bad image count");
    if (!images) return fail(CVO_ERR_INVALID, "null argument: images");
    if (!image_size_ok(width, height)) return fail(CVO_ERR_INVALID, "image size out of range");
    for (int k = 0; k < count; ++k) {
        const cvo_device_image& im = images[k];
        const std::string who = "image " + std::to_string(k) + ": ";
        if (!im.bgr8) return fail(CVO_ERR_INVALID, who + "bgr8 is null");
        if (!im.depth16) return fail(CVO_ERR_INVALID, who + "depth16 is null");
        if (im.pixel_bytes != 3 && im.pixel_bytes != 4) return fail(CVO_ERR_INVALID, who + "pixel_bytes must be 3 or 4, got " + std::to_string(im.pixel_bytes));
        if (im.swap_rb != 0 && im.swap_rb != 1) return fail(CVO_ERR_INVALID, who + "swap_rb must be 0 or 1, got " + std::to_string(im.swap_rb));
        const long long row = (long long)width * im.pixel_bytes, drow = 2ll * width;
        if (im.bgr_pitch < 0 || (im.bgr_pitch != 0 && im.bgr_pitch < row)) return fail(CVO_ERR_INVALID, who + "bgr_pitch " + std::to_string(im.bgr_pitch) + " is below the row's " + std::to_string(row) + " bytes");
        if (im.depth_pitch < 0 || (im.depth_pitch != 0 && im.depth_pitch < drow)) return fail(CVO_ERR_INVALID, who + "depth_pitch " + std::to_string(im.depth_pitch) + " is below the row's " + std::to_string(drow) + " bytes");
        if (reinterpret_cast<uintptr_t>(im.depth16) & 1u) return fail(CVO_ERR_INVALID, who + "depth16 is not 2-byte aligned");
        if (im.depth_pitch & 1) return fail(CVO_ERR_INVALID, who + "depth_pitch is not a multiple of 2");
    }
    HIP_TRY(hipSetDevice(device));
    for (int k = 0; k < count; ++k) {
        const cvo_device_image& im = images[k];
        const std::string who = "image " + std::to_string(k) + ": ";
        const long long row = (long long)width * im.pixel_bytes, drow = 2ll * width;
        int rc;
        if ((rc = check_device_plane(device, im.bgr8, im.bgr_pitch ? im.bgr_pitch : row, row, height, who + "bgr8"))) return rc;
        if ((rc = check_device_plane(device, im.depth16, im.depth_pitch ? im.depth_pitch : drow, drow, height, who + "depth16"))) return rc;
    }
    return CVO_OK;
}

// ---- the stage: the next step's frames generated ahead, on a stream of their own (FrameStage)
void pool_free_cloud(std::vector<std::shared_ptr<Cloud>>& pool, std::shared_ptr<Cloud>& out) {
    for (std::shared_ptr<Cloud>& c : pool) if (c.use_count() == 1) { out = c; return; }
    pool.push_back(std::make_shared<Cloud>());
    out = pool.back();
}
// The stage stream is made with the highest priority the device has.  HIP deals streams of one priority onto the process's few hardware queues in turn,
// and a stream that lands on the queue of a persistent align launch makes no progress until that launch ends; priority streams take their queues
// from a set of their own, so the generator's copies and kernels start while the launch runs (on the CUs it leaves free) instead of behind it.
int stage_ready(cvo_batch b) {
    FrameStage& F = b->stage;
    if (F.s) return CVO_OK;
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamCreateWithPriority(&F.s, hipStreamNonBlocking, greatest));
    HIP_TRY(hipEventCreateWithFlags(&F.ev_gen, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&F.ev_done, hipEventDisableTiming));
    if (!F.pool) F.pool = &b->pool;
    return CVO_OK;
}
// the staged list is given up: its cloud objects are free again (only the pool holds them).  Work of it that is still queued runs to its end on the
// stage stream; the next stage call is ordered behind it there and waits for its copies before it writes the pinned stage again.
void stage_drop(cvo_batch b) {
    FrameStage& F = b->stage;
    F.pending = F.placed = false; F.rc = CVO_OK; F.err.clear();
    F.list.clear(); F.points.clear(); F.clouds.clear();
}
void stage_drop_if_listed(cvo_batch b, int p) {
    FrameStage& F = b->stage;
    if (F.pending && std::find(F.list.begin(), F.list.end(), p) != F.list.end()) stage_drop(b);
}
// `count` images staged for the slots / streams of `list` (the arguments are checked): returns with everything queued and every image byte copied
int stage_begin(cvo_batch b, int count, const int* list, const ImageSrc& src, int width, int height,
                const cvo_camera* cams, const int* cam_index) {
    Lap lap(StepLaps::STAGE);
    Engine& E = b->eng; FrameStage& F = b->stage;
    HIP_TRY(hipSetDevice(E.device));
    int rc = stage_ready(b); if (rc) return rc;
    F.img.num_want = b->img.num_want;
    // an earlier stage's copies read the pinned stage this call writes, its read-back writes the records this call's placing reads
    if (!F.gen_waited) { F.gen_waited = true; HIP_TRY(hipEventSynchronize(F.ev_gen)); }
    stage_drop(b);                                                   // (a stage that was never consumed is replaced)
    std::vector<cvo_camera> cam_of(count);
    for (int k = 0; k < count; ++k) cam_of[k] = cams[cam_index ? cam_index[k] : 0];
    rc = generate_enqueue(E, F.img, F.s, count, src, width, height, nullptr, cam_of.data(), E.upload_threads);
    if (rc) { (void)hipStreamSynchronize(F.s); return rc; }         // (nothing of a failed call stays in flight)
    HIP_TRY(hipEventRecord(F.ev_gen, F.s));
    F.gen_waited = false;
    F.list.assign(list, list + count);
    F.pending = true;
    return CVO_OK;
}
// The staged clouds into cloud objects nobody holds, with their boxes: needs the point counts, so the generator must have finished.  block: wait
// for it; else only when it already has.  What goes wrong here (a cloud above 65 535 points, a HIP error of the staged work) is kept for the
// consuming call to report.  The objects are free ones of the pool: no queued or running launch reads them -- a launch only reads clouds that
// slots held when it was set up, and a slot's object returns to the pool (commit, wait, the next step's hand-over) after its launch was waited for.
int stage_place(cvo_batch b, bool block) {
    Engine& E = b->eng; FrameStage& F = b->stage;
    if (!F.pending || F.placed) return CVO_OK;
    HIP_TRY(hipSetDevice(E.device));
    if (!block) {
        const hipError_t q = hipEventQuery(F.ev_gen);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return CVO_OK; }
    }
    F.placed = true;
    const hipError_t es = hipEventSynchronize(F.ev_gen);
    F.gen_waited = true;
    if (es != hipSuccess) { (void)hipGetLastError(); F.rc = CVO_ERR_HIP; F.err = std::string("staged frames: ") + hipGetErrorString(es); return CVO_OK; }
    const int N = (int)F.list.size(), cap = PCD_CLOUD_CAP;
    const PcdImgRec* R = static_cast<const PcdImgRec*>(F.img.h_rec.p);
    if (check_cloud_caps(R, N) != CVO_OK) { F.rc = CVO_ERR_INVALID; F.err = g_err; return CVO_OK; }
    auto bad = [&](int rc) { F.rc = rc; F.err = g_err; F.clouds.clear(); return CVO_OK; };
    int rc;
    if ((rc = F.h_box.ensure(sizeof(BoxDesc) * (size_t)N))) return bad(rc);
    BoxDesc* bd = static_cast<BoxDesc*>(F.h_box.p);
    F.clouds.assign(N, nullptr); F.points.assign(N, 0);
    PcdScatter sc; std::memset(&sc, 0, sizeof(sc));
    sc.src = (const float*)F.img.cloud.p; sc.src_px = (const uint16_t*)F.img.px.p; sc.rec = (const PcdImgRec*)F.img.rec.p; sc.cap = cap;
    int n_max = 0, n_box = 0, box_max = 0;
    auto flush = [&]() -> int {
        const hipError_t e = pcd_launch_scatter(sc, n_max, F.s);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("pcd scatter: ") + hipGetErrorString(e));
        sc.n = 0; n_max = 0; return CVO_OK;
    };
    for (int k = 0; k < N; ++k) {
        pool_free_cloud(*F.pool, F.clouds[k]);
        Cloud& c = *F.clouds[k];
        const PcdImgRec& r = R[k];
        F.points[k] = r.npts;
        c.n = r.npts; c.n_px = r.npts; c.boxes_valid = false; c.raw = nullptr; c.raw_feat = nullptr; c.multi = false;
        c.cost_hint = r.cost_n > 0 ? (float)(r.cost / r.cost_n) : 0.f;
        if (c.n <= 0) continue;
        if ((rc = c.buf.ensure((size_t)c.n * REC * sizeof(float))) || (rc = c.px.ensure((size_t)c.n * 2 * sizeof(uint16_t))) || (rc = c.boxes.ensure(score_box_bytes(c.n)))) return bad(rc);
        sc.img[sc.n] = k; sc.dst[sc.n] = c.rec(); sc.dst_px[sc.n] = (uint16_t*)c.px.p; ++sc.n; n_max = std::max(n_max, c.n);
        if (sc.n == PCD_SCATTER_MAX && (rc = flush())) return bad(rc);
        BoxDesc& D = bd[n_box++];
        D.rec = c.rec(); D.gbox = static_cast<float*>(c.boxes.p); D.self_cache = score_self_cache(D.gbox, c.n); D.n = c.n; D.ngroups = score_groups(c.n);
        box_max = std::max(box_max, c.n);
        c.boxes_valid = true; c.boxes_stream = E.stream;             // (the engine's stream is ordered behind ev_done before anything uses them: stage_take)
    }
    if (sc.n > 0 && (rc = flush())) return bad(rc);
    const hipError_t e = launch_cloud_boxes_batch(bd, n_box, box_max, F.s);
    if (e != hipSuccess) return bad(fail(CVO_ERR_HIP, std::string("cloud box kernel launch: ") + hipGetErrorString(e)));
    const hipError_t er = hipEventRecord(F.ev_done, F.s);
    if (er != hipSuccess) return bad(fail(CVO_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(er)));
    return CVO_OK;
}
// The consuming call's first half: the staged clouds are placed (waiting for the generator if it has not finished), an error of the staged work
// is reported and drops the stage.  On success F.clouds / F.points are the listed frames' clouds, and the engine's stream waits for them by an
// event: launches on it follow without a host wait, a launch on another stream waits for the engine's stream once (Engine::settle_uploads).
int stage_take(cvo_batch b) {
    FrameStage& F = b->stage;
    int rc = stage_place(b, true); if (rc) return rc;
    if (F.rc != CVO_OK) { const int code = F.rc; const std::string msg = F.err; stage_drop(b); return fail(code, msg); }
    HIP_TRY(hipStreamWaitEvent(b->eng.stream, F.ev_done, 0));
    b->eng.uploads_pending = true;
    return CVO_OK;
}
void stage_taken(cvo_batch b) { FrameStage& F = b->stage; F.taken += (long long)F.list.size(); stage_drop(b); }
void stage_destroy(cvo_batch b) {
    FrameStage& F = b->stage;
    if (F.s) (void)hipStreamSynchronize(F.s);
    stage_drop(b);
    F.img.release(); F.h_box.release();
    if (F.ev_gen) (void)hipEventDestroy(F.ev_gen);
    if (F.ev_done) (void)hipEventDestroy(F.ev_done);
    if (F.s) (void)hipStreamDestroy(F.s);
    F.s = nullptr; F.ev_gen = F.ev_done = nullptr;
}
int stage_count(cvo_batch b, int* images, long long* taken) {
    if (images) *images = b->stage.pending ? (int)b->stage.list.size() : 0;
    if (taken) *taken = b->stage.taken;
    return CVO_OK;
}
}  // namespace

namespace {
int batch_set_pairs_from(cvo_batch b, int first, int count, int n_images, const ImageSrc& src,
                         int width, int height, const cvo_camera* cam, const int* fixed_image, const int* moving_image, int* points_out) {
    if (!b || first < 0 || count <= 0 || first + count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad pair range");
    if ((!src.dev && (!src.bgr8 || !src.depth16)) || !cam || !fixed_image || !moving_image) return fail(CVO_ERR_INVALID, "null argument");
    if (n_images <= 0 || n_images > 65535) return fail(CVO_ERR_INVALID, "bad image count");
    if (!image_size_ok(width, height)) return fail(CVO_ERR_INVALID, "image size out of range");
    if (!src.dev) for (int k = 0; k < n_images; ++k) if (!src.bgr8[k] || !src.depth16[k]) return fail(CVO_ERR_INVALID, "null image pointer");
    for (int k = 0; k < count; ++k)
        if (fixed_image[k] < 0 || fixed_image[k] >= n_images || moving_image[k] < 0 || moving_image[k] >= n_images) return fail(CVO_ERR_INVALID, "image index out of range");
    int rc = batch_settle(b); if (rc) return rc;
    const PcdImgRec* R = nullptr;
    if ((rc = batch_generate(b, n_images, src, width, height, cam, nullptr, &R))) return rc;
    // commit: the pairs take their clouds
    std::vector<Cloud*> dst; std::vector<int> img;
    for (int k = 0; k < count; ++k) {
        const int p = first + k;
        end_stream(b, p);
        own_slot_clouds(b, p);
        if (!b->fixed[p]) b->fixed[p].reset(new Cloud());
        if (!b->moving[p]) b->moving[p].reset(new Cloud());
        dst.push_back(b->fixed[p].get()); img.push_back(fixed_image[k]);
        dst.push_back(b->moving[p].get()); img.push_back(moving_image[k]);
    }
    if ((rc = batch_scatter(b, dst, img, R))) return rc;
    for (int k = 0; k < count; ++k) fresh_state(b->init_states[first + k], b->prm.ell);
    states_dirty(b);
    if (points_out) for (int k = 0; k < n_images; ++k) points_out[k] = R[k].npts;
    return CVO_OK;
}
int batch_check_images(cvo_batch b, int count, const int* slots, const ImageSrc& src, int width, int height, const cvo_camera* cams, const int* cam_index) {
    if (!b || count <= 0 || count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad image count");
    if (!slots || (!src.dev && (!src.bgr8 || !src.depth16)) || !cams) return fail(CVO_ERR_INVALID, "null argument");
    if (!image_size_ok(width, height)) return fail(CVO_ERR_INVALID, "image size out of range");
    std::vector<unsigned char> seen(b->max_pairs, 0);
    for (int k = 0; k < count; ++k) {
        if (slots[k] < 0 || slots[k] >= b->max_pairs) return fail(CVO_ERR_INVALID, "slot index out of range");
        if (seen[slots[k]]++) return fail(CVO_ERR_INVALID, "slot listed twice");
        if (!src.dev && (!src.bgr8[k] || !src.depth16[k])) return fail(CVO_ERR_INVALID, "null image pointer");
        if (cam_index && cam_index[k] < 0) return fail(CVO_ERR_INVALID, "camera index out of range");
    }
    return CVO_OK;
}
// ---- K-stream odometry: slot p is one cvo::cvo object that takes a frame per call (cvo_main's loop, cvo.cpp:352-386 + 461-473 + 578-582)
int batch_advance_from(cvo_batch b, int count, const int* slots, const ImageSrc& src, int width, int height,
                       const cvo_camera* cams, const int* cam_index, int* points_out) {
    int rc = batch_check_images(b, count, slots, src, width, height, cams, cam_index); if (rc) return rc;
    if ((rc = batch_settle(b))) return rc;
    std::vector<cvo_camera> cam_of(count);
    for (int k = 0; k < count; ++k) cam_of[k] = cams[cam_index ? cam_index[k] : 0];
    const PcdImgRec* R = nullptr;
    if ((rc = batch_generate(b, count, src, width, height, nullptr, cam_of.data(), &R))) return rc;   // (fails before any slot changes)
    // commit.  A started slot's moving cloud becomes its fixed cloud by a move of ownership (update_fixed_pcd, cvo.cpp:578-582); the cloud object it
    // held as the fixed one is taken for the new moving cloud, whose points the scatter overwrites (its boxes and cached self products are dropped)
    std::vector<Cloud*> dst; std::vector<int> img;
    for (int k = 0; k < count; ++k) {
        const int p = slots[k];
        own_slot_clouds(b, p);
        if (!b->fixed[p]) b->fixed[p].reset(new Cloud());
        if (!b->moving[p]) b->moving[p].reset(new Cloud());
        if (!b->streams[p].on) fresh_stream(b, p);
        StreamSlot& S = b->streams[p];
        slot_clouds_changed(b, p);
        if (!S.init) {                                                // cvo.cpp:352-360: the first frame only fills the fixed cloud
            S.init = true;
            dst.push_back(b->fixed[p].get());
        } else {
            if (S.has_moving) std::swap(b->fixed[p], b->moving[p]);
            S.has_moving = true;
            dst.push_back(b->moving[p].get());
        }
        img.push_back(k);
    }
    if ((rc = batch_scatter(b, dst, img, R))) return rc;
    if (points_out) for (int k = 0; k < count; ++k) points_out[k] = R[k].npts;
    return CVO_OK;
}
}  // namespace
int cvo_batch_set_pairs_images(cvo_batch b, int first, int count, int n_images, const unsigned char* const* bgr8, const unsigned short* const* depth16,
                               int width, int height, const cvo_camera* cam, const int* fixed_image, const int* moving_image, int* points_out) {
    return batch_set_pairs_from(b, first, count, n_images, ImageSrc::host(bgr8, depth16), width, height, cam, fixed_image, moving_image, points_out);
}
int cvo_batch_set_pairs_device_images(cvo_batch b, int first, int count, int n_images, const cvo_device_image* images, int width, int height,
                                      const cvo_camera* cam, const int* fixed_image, const int* moving_image, int* points_out, void* image_stream) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    int rc = check_device_images(b->eng.device, n_images, images, width, height); if (rc) return rc;
    return batch_set_pairs_from(b, first, count, n_images, ImageSrc::device(images, image_stream), width, height, cam, fixed_image, moving_image, points_out);
}
int cvo_batch_advance_images(cvo_batch b, int count, const int* slots, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                             const cvo_camera* cams, const int* cam_index, int* points_out) {
    return batch_advance_from(b, count, slots, ImageSrc::host(bgr8, depth16), width, height, cams, cam_index, points_out);
}
int cvo_batch_advance_device_images(cvo_batch b, int count, const int* slots, const cvo_device_image* images, int width, int height,
                                    const cvo_camera* cams, const int* cam_index, int* points_out, void* image_stream) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    int rc = check_device_images(b->eng.device, count, images, width, height); if (rc) return rc;
    return batch_advance_from(b, count, slots, ImageSrc::device(images, image_stream), width, height, cams, cam_index, points_out);
}
int cvo_batch_reset_stream(cvo_batch b, int p) {
    if (!b || p < 0 || p >= b->max_pairs) return fail(CVO_ERR_INVALID, "bad slot index");
    int rc = batch_settle(b); if (rc) return rc;
    if (b->eng.launched && b->eng.last_stream) HIP_TRY(hipStreamSynchronize(b->eng.last_stream));   // (a launch may still read the clouds; their memory is kept)
    slot_clouds_changed(b, p);
    own_slot_clouds(b, p);
    fresh_stream(b, p);
    return CVO_OK;
}
// ---- the next frames of stream slots staged ahead: generated on a stream of the stage's own while a launch runs, taken by cvo_batch_advance_staged
int cvo_batch_stage_images(cvo_batch b, int count, const int* slots, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                           const cvo_camera* cams, const int* cam_index) {
    const ImageSrc src = ImageSrc::host(bgr8, depth16);
    int rc = batch_check_images(b, count, slots, src, width, height, cams, cam_index); if (rc) return rc;   // (an earlier stage survives a refused call)
    return stage_begin(b, count, slots, src, width, height, cams, cam_index);
}
int cvo_batch_stage_device_images(cvo_batch b, int count, const int* slots, const cvo_device_image* images, int width, int height,
                                  const cvo_camera* cams, const int* cam_index, void* image_stream) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    int rc = check_device_images(b->eng.device, count, images, width, height); if (rc) return rc;
    const ImageSrc src = ImageSrc::device(images, image_stream);
    if ((rc = batch_check_images(b, count, slots, src, width, height, cams, cam_index))) return rc;
    return stage_begin(b, count, slots, src, width, height, cams, cam_index);
}
int cvo_check_device_images(int device, int count, const cvo_device_image* images, int width, int height) {
    return check_device_images(device, count, images, width, height);
}
// The ingest kernel alone (tests): `count` images into packed stacks that lie between guard bytes; the stacks and the guards' state come back.
int cvo_selftest_ingest_images(int device, int count, const cvo_device_image* images, int width, int height, unsigned char* bgr_out, unsigned short* depth_out,
                               int* guards_intact) {
    if (!bgr_out || !depth_out || !guards_intact) return fail(CVO_ERR_INVALID, "null argument");
    int rc = check_device_images(device, count, images, width, height); if (rc) return rc;
    constexpr size_t G = 64;
    const size_t n = (size_t)width * height, nb = 3 * n * count, nd = 2 * n * count;
    DevBuf bb, db;
    BatchImages T; T.n_cap = count;                                   // (only the ingest's table and events; the stacks start behind the front guards)
    struct Release { DevBuf& bb; DevBuf& db; BatchImages& T; ~Release() { T.bgr.p = nullptr; T.depth.p = nullptr; T.release(); bb.release(); db.release(); } } release{bb, db, T};
    if ((rc = bb.ensure(nb + 2 * G)) || (rc = db.ensure(nd + 2 * G))) return rc;
    HIP_TRY(hipMemset(bb.p, 0xA5, nb + 2 * G));
    HIP_TRY(hipMemset(db.p, 0xA5, nd + 2 * G));
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct Close { hipStream_t s; ~Close() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } close_{s};
    unsigned char* b0 = static_cast<unsigned char*>(bb.p); unsigned char* d0 = static_cast<unsigned char*>(db.p);
    T.bgr.p = b0 + G; T.depth.p = d0 + G;
    ImageSrc src; src.dev = images;
    if ((rc = ingest_enqueue(T, s, count, src, width, height))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned char> gb(2 * G), gd(2 * G);
    HIP_TRY(hipMemcpy(bgr_out, b0 + G, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(depth_out, d0 + G, nd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(gb.data(), b0, G, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(gb.data() + G, b0 + G + nb, G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(gd.data(), d0, G, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(gd.data() + G, d0 + G + nd, G, hipMemcpyDeviceToHost));
    int ok = 1;
    for (unsigned char v : gb) ok &= v == 0xA5;
    for (unsigned char v : gd) ok &= v == 0xA5;
    *guards_intact = ok;
    return CVO_OK;
}
// ---- clouds that are already on the GPU (cvo_device_cloud): the device twin of the cloud hand-over.  Eager: one ingest launch per call copies
// the caller's arrays into library-owned cloud objects, one box launch behind it makes their group boxes; from there on they are clouds like any other.
namespace {
void cloud_strides(const cvo_device_cloud& c, long long* xs, long long* ps, long long* cs) {
    *xs = c.xyz_stride ? c.xyz_stride : 12;
    const bool ref = c.feat_point_stride == 0 && c.feat_channel_stride == 0;         // the reference layout: 5 channel-major arrays of n (data_type.h:75)
    *ps = ref ? 4 : c.feat_point_stride; *cs = ref ? 4ll * c.n : c.feat_channel_stride;
}
// What every device-cloud entry point checks first, before any slot or stream changes and before anything is queued (cvo_check_device_clouds runs it alone).
// n_limit: 65535 for a hand-over (16-bit column indices), CVO_REDUCE_MAX_POINTS in front of a reducer.
// names: what to call cloud k in a message instead of "cloud k: " (a fusion's "group g member m: ").
int check_device_clouds(int device, int count, const cvo_device_cloud* clouds, int n_limit = 65535, const std::string* names = nullptr) {
    if (count <= 0 || count > 65535) return fail(CVO_ERR_INVALID, "bad cloud count");
    if (!clouds) return fail(CVO_ERR_INVALID, "null argument: clouds");
    for (int k = 0; k < count; ++k) {
        const cvo_device_cloud& c = clouds[k];
        const std::string who = names ? names[k] : "cloud " + std::to_string(k) + ": ";
        if (c.n < 0 || c.n > n_limit)
            return fail(CVO_ERR_INVALID, who + "n " + std::to_string(c.n) + " is outside 0 .. " + std::to_string(n_limit) + (n_limit == 65535 ? " (16-bit column indices)" : ""));
        const struct { const char* name; long long v; } strides[3] = {{"xyz_stride", c.xyz_stride}, {"feat_point_stride", c.feat_point_stride}, {"feat_channel_stride", c.feat_channel_stride}};
        for (const auto& st : strides) {
            if (st.v < 0) return fail(CVO_ERR_INVALID, who + st.name + " " + std::to_string(st.v) + " is negative");
            if (st.v & 3) return fail(CVO_ERR_INVALID, who + st.name + " " + std::to_string(st.v) + " is not a multiple of 4");
            if (st.v > (1ll << 40)) return fail(CVO_ERR_INVALID, who + st.name + " " + std::to_string(st.v) + " is out of range");
        }
        if (c.xyz_stride != 0 && c.xyz_stride < 12) return fail(CVO_ERR_INVALID, who + "xyz_stride " + std::to_string(c.xyz_stride) + " is below a point's 12 bytes");
        if ((c.feat_point_stride == 0) != (c.feat_channel_stride == 0)) return fail(CVO_ERR_INVALID, who + "exactly one of feat_point_stride and feat_channel_stride is 0");
        if (c.n == 0) continue;                                       // (an empty cloud needs no pointers)
        if (!c.xyz) return fail(CVO_ERR_INVALID, who + "xyz is null");
        if (!c.feat) return fail(CVO_ERR_INVALID, who + "feat is null");
        if (reinterpret_cast<uintptr_t>(c.xyz) & 3u) return fail(CVO_ERR_INVALID, who + "xyz is not 4-byte aligned");
        if (reinterpret_cast<uintptr_t>(c.feat) & 3u) return fail(CVO_ERR_INVALID, who + "feat is not 4-byte aligned");
    }
    HIP_TRY(hipSetDevice(device));
    for (int k = 0; k < count; ++k) {
        const cvo_device_cloud& c = clouds[k];
        if (c.n == 0) continue;
        const std::string who = names ? names[k] : "cloud " + std::to_string(k) + ": ";
        long long xs, ps, cs; cloud_strides(c, &xs, &ps, &cs);
        int rc;
        if ((rc = check_device_plane(device, c.xyz, xs, 12, c.n, who + "xyz", "cloud"))) return rc;              // [xyz, xyz + (n-1)*xyz_stride + 12)
        if ((rc = check_device_plane(device, c.feat, ps, 4 * cs + 4, c.n, who + "feat", "cloud"))) return rc;    // [feat, feat + (n-1)*point_stride + 4*channel_stride + 4)
    }
    return CVO_OK;
}
// One cloud of an ingest launch (n > 0): where it goes, where its boxes go (null: none are made), and what its cost samples came to.
struct IngestItem { const cvo_device_cloud* src; float* dst; float* gbox; double cost_sum; int cost_n; };
// ONE ingest launch for all items on s, a stream of the library's own (see ingest_enqueue: a caller's stream may sit behind a persistent launch),
// and ONE box launch behind it.  With a cloud_stream: s waits for what is queued there by an event, and the cloud_stream waits for the ingest by a
// second one.  The host waits for the ingest alone, always: the cost samples its blocks wrote to pinned memory are added up here, in block order.
int ingest_clouds_run(CloudIntake& C, hipStream_t s, hipStream_t cloud_stream, std::vector<IngestItem>& items) {
    const int live = (int)items.size();
    if (live == 0) return CVO_OK;
    int rc;
    for (hipEvent_t* e : {&C.ev_in, &C.ev_out, &C.ev_box[0], &C.ev_box[1]}) if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    size_t blocks = 0; int n_max = 0;
    for (const IngestItem& it : items) { blocks += (size_t)(it.src->n + 255) / 256; n_max = std::max(n_max, it.src->n); }
    const int f = C.flip; C.flip ^= 1;
    if (C.box_queued[f]) { HIP_TRY(hipEventSynchronize(C.ev_box[f])); C.box_queued[f] = false; }   // (the box launch before the last one: long over)
    if ((rc = C.h_desc.ensure(sizeof(CloudIngestDesc) * (size_t)live)) || (rc = C.h_cost.ensure(sizeof(double) * 2 * blocks)) || (rc = C.h_box[f].ensure(sizeof(BoxDesc) * (size_t)live))) return rc;
    CloudIngestDesc* d = static_cast<CloudIngestDesc*>(C.h_desc.p);
    BoxDesc* bd = static_cast<BoxDesc*>(C.h_box[f].p);
    double* cost = static_cast<double*>(C.h_cost.p);
    size_t at = 0; int n_box = 0;
    for (int q = 0; q < live; ++q) {
        const cvo_device_cloud& c = *items[q].src;
        long long xs, ps, cs; cloud_strides(c, &xs, &ps, &cs);
        d[q].xyz = static_cast<const float*>(c.xyz); d[q].feat = static_cast<const float*>(c.feat); d[q].dst = items[q].dst; d[q].cost = cost + 2 * at;
        d[q].xyz_stride = xs; d[q].feat_point_stride = ps; d[q].feat_channel_stride = cs; d[q].n = c.n; d[q].xyz_tight = xs == 12;
        at += (size_t)(c.n + 255) / 256;
        if (items[q].gbox) {
            BoxDesc& D = bd[n_box++];
            D.rec = items[q].dst; D.gbox = items[q].gbox; D.self_cache = score_self_cache(D.gbox, c.n); D.n = c.n; D.ngroups = score_groups(c.n);
        }
    }
    if (cloud_stream) {
        HIP_TRY(hipEventRecord(C.ev_in, cloud_stream));
        HIP_TRY(hipStreamWaitEvent(s, C.ev_in, 0));
    }
    hipError_t e = launch_ingest_clouds(d, live, n_max, s);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("cloud ingest kernel launch: ") + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(C.ev_out, s));
    if (n_box > 0) {
        e = launch_cloud_boxes_batch(bd, n_box, n_max, s);
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("cloud box kernel launch: ") + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(C.ev_box[f], s));
        C.box_queued[f] = true;
    }
    if (cloud_stream) HIP_TRY(hipStreamWaitEvent(cloud_stream, C.ev_out, 0));
    {
        Lap lap(StepLaps::INGEST);
        HIP_TRY(hipEventSynchronize(C.ev_out));                       // (the call's one host wait)
    }
    at = 0;
    for (int q = 0; q < live; ++q) {
        const size_t nb = (size_t)(items[q].src->n + 255) / 256;
        double sum = 0.0, m = 0.0;
        for (size_t k = 0; k < nb; ++k) { sum += cost[2 * (at + k)]; m += cost[2 * (at + k) + 1]; }
        items[q].cost_sum = sum; items[q].cost_n = (int)m;
        at += nb;
    }
    return CVO_OK;
}
// `count` checked clouds into cloud objects of `pool` that nothing else holds (out[k]; an empty cloud gets an empty object), on b's stream.  No slot
// changes.  A free object is read by no launch that is queued behind this call's work: the launches of b run on its stream, or are waited for here.
int clouds_ingest(cvo_batch b, std::vector<std::shared_ptr<Cloud>>& pool, int count, const cvo_device_cloud* clouds, void* cloud_stream,
                  std::vector<std::shared_ptr<Cloud>>& out) {
    Engine& E = b->eng;
    HIP_TRY(hipSetDevice(E.device));
    if (E.launched && E.last_stream && E.last_stream != E.stream) HIP_TRY(hipStreamSynchronize(E.last_stream));
    out.assign(count, nullptr);
    std::vector<IngestItem> items; std::vector<int> of; items.reserve(count); of.reserve(count);
    int rc;
    for (int k = 0; k < count; ++k) {
        pool_free_cloud(pool, out[k]);
        Cloud& c = *out[k];
        c.n = clouds[k].n; c.n_px = 0; c.boxes_valid = false; c.raw = nullptr; c.raw_feat = nullptr; c.cost_hint = 0.f; c.multi = false;
        if (c.n <= 0) continue;
        if ((rc = c.buf.ensure((size_t)c.n * REC * sizeof(float))) || (rc = c.boxes.ensure(score_box_bytes(c.n)))) return rc;
        items.push_back(IngestItem{&clouds[k], c.rec(), static_cast<float*>(c.boxes.p), 0.0, 0}); of.push_back(k);
    }
    if ((rc = ingest_clouds_run(b->cin, E.stream, static_cast<hipStream_t>(cloud_stream), items))) return rc;
    for (size_t q = 0; q < items.size(); ++q) {
        Cloud& c = *out[of[q]];
        c.cost_hint = items[q].cost_n > 0 ? (float)(items[q].cost_sum / items[q].cost_n) : 0.f;
        c.boxes_valid = true; c.boxes_stream = E.stream;
    }
    E.uploads_pending = true;                                         // (a launch on another stream waits for the engine's stream once: settle_uploads)
    return CVO_OK;
}
}  // namespace
int cvo_check_device_clouds(int device, int count, const cvo_device_cloud* clouds) { return check_device_clouds(device, count, clouds); }
int cvo_batch_set_pairs_device_clouds(cvo_batch b, int first, int count, int n_clouds, const cvo_device_cloud* clouds, const int* fixed_cloud, const int* moving_cloud,
                                      void* cloud_stream) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (first < 0 || count <= 0 || first + count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad pair range");
    if (!fixed_cloud || !moving_cloud) return fail(CVO_ERR_INVALID, "null argument");
    int rc = check_device_clouds(b->eng.device, n_clouds, clouds); if (rc) return rc;
    for (int k = 0; k < count; ++k)
        if (fixed_cloud[k] < 0 || fixed_cloud[k] >= n_clouds || moving_cloud[k] < 0 || moving_cloud[k] >= n_clouds) return fail(CVO_ERR_INVALID, "cloud index out of range");
    if ((rc = batch_settle(b))) return rc;
    std::vector<std::shared_ptr<Cloud>> in;
    if ((rc = clouds_ingest(b, b->pool, n_clouds, clouds, cloud_stream, in))) return rc;   // (fails before any pair changes)
    // commit: the pairs take the cloud objects; one listed for several pairs is held by all of them
    if (b->eng.launched && b->eng.last_stream) HIP_TRY(hipStreamSynchronize(b->eng.last_stream));   // (objects the pairs give up are written by later hand-overs)
    std::vector<int> uses(n_clouds, 0);
    for (int k = 0; k < count; ++k) { ++uses[fixed_cloud[k]]; ++uses[moving_cloud[k]]; }
    for (int j = 0; j < n_clouds; ++j) in[j]->multi = uses[j] > 1;
    auto give_up = [&](std::shared_ptr<Cloud>& c) { if (c && c.use_count() == 1) b->pool.push_back(c); c.reset(); };
    for (int k = 0; k < count; ++k) {
        const int p = first + k;
        end_stream(b, p);
        give_up(b->fixed[p]); give_up(b->moving[p]);
        b->fixed[p] = in[fixed_cloud[k]]; b->moving[p] = in[moving_cloud[k]];
        fresh_state(b->init_states[p], b->prm.ell);
    }
    states_dirty(b);
    return CVO_OK;
}
int cvo_batch_advance_device_clouds(cvo_batch b, int count, const int* slots, const cvo_device_cloud* clouds, void* cloud_stream) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (count <= 0 || count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad cloud count");
    if (!slots) return fail(CVO_ERR_INVALID, "null argument");
    int rc = check_device_clouds(b->eng.device, count, clouds); if (rc) return rc;
    std::vector<unsigned char> seen(b->max_pairs, 0);
    for (int k = 0; k < count; ++k) {
        if (slots[k] < 0 || slots[k] >= b->max_pairs) return fail(CVO_ERR_INVALID, "slot index out of range");
        if (seen[slots[k]]++) return fail(CVO_ERR_INVALID, "slot listed twice");
    }
    if ((rc = batch_settle(b))) return rc;
    std::vector<std::shared_ptr<Cloud>> in;
    if ((rc = clouds_ingest(b, b->pool, count, clouds, cloud_stream, in))) return rc;      // (fails before any slot changes)
    if (b->eng.launched && b->eng.last_stream) HIP_TRY(hipStreamSynchronize(b->eng.last_stream));   // (as cvo_batch_advance_staged: objects the slots give up are written later)
    auto give_up = [&](std::shared_ptr<Cloud>& c) { if (c && c.use_count() == 1) b->pool.push_back(c); c.reset(); };
    for (int k = 0; k < count; ++k) {                                // the commit of cvo_batch_advance_staged
        const int p = slots[k];
        stage_drop_if_listed(b, p);
        own_slot_clouds(b, p);
        if (!b->streams[p].on) fresh_stream(b, p);
        StreamSlot& S = b->streams[p];
        slot_clouds_changed(b, p);
        if (!S.init) {                                                // cvo.cpp:352-360: the first cloud only fills the fixed slot
            S.init = true;
            give_up(b->fixed[p]); b->fixed[p] = in[k];
            if (!b->moving[p]) b->moving[p].reset(new Cloud());
        } else {
            if (S.has_moving) { give_up(b->fixed[p]); b->fixed[p] = b->moving[p]; b->moving[p].reset(); }   // update_fixed_pcd, cvo.cpp:578-582
            else give_up(b->moving[p]);
            S.has_moving = true;
            b->moving[p] = in[k];
        }
    }
    return CVO_OK;
}
// The ingest kernel alone (tests): every cloud's planes lie between 64 guard bytes on either side, prefilled with 0xA5
int cvo_selftest_ingest_clouds(int device, int count, const cvo_device_cloud* clouds, float* xyz_out, float* feat_out, double* cost_out, int* guards_intact) {
    if (!xyz_out || !feat_out || !cost_out || !guards_intact) return fail(CVO_ERR_INVALID, "null argument");
    int rc = check_device_clouds(device, count, clouds); if (rc) return rc;
    constexpr size_t G = 64;
    size_t bytes = G;
    for (int k = 0; k < count; ++k) bytes += (size_t)clouds[k].n * REC * sizeof(float) + G;
    DevBuf buf; CloudIntake C;
    struct Release { DevBuf& b; CloudIntake& C; ~Release() { C.release(); b.release(); } } release{buf, C};
    if ((rc = buf.ensure(bytes))) return rc;
    HIP_TRY(hipMemset(buf.p, 0xA5, bytes));
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct Close { hipStream_t s; ~Close() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } close_{s};
    unsigned char* base = static_cast<unsigned char*>(buf.p);
    std::vector<IngestItem> items; std::vector<int> of;
    size_t at = G;
    for (int k = 0; k < count; ++k) {
        if (clouds[k].n > 0) { items.push_back(IngestItem{&clouds[k], reinterpret_cast<float*>(base + at), nullptr, 0.0, 0}); of.push_back(k); }
        at += (size_t)clouds[k].n * REC * sizeof(float) + G;
    }
    if ((rc = ingest_clouds_run(C, s, nullptr, items))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned char> host(bytes);
    HIP_TRY(hipMemcpy(host.data(), buf.p, bytes, hipMemcpyDeviceToHost));
    for (int k = 0; k < count; ++k) { cost_out[2 * k] = 0.0; cost_out[2 * k + 1] = 0.0; }
    for (size_t q = 0; q < items.size(); ++q) { cost_out[2 * of[q]] = items[q].cost_sum; cost_out[2 * of[q] + 1] = (double)items[q].cost_n; }
    int ok = 1;
    auto guard = [&](size_t from) { for (size_t i = 0; i < G; ++i) ok &= host[from + i] == 0xA5; };
    at = 0; guard(at); at += G;
    for (int k = 0; k < count; ++k) {                                // the planes back to the reference layout: n x 3 positions, 5 channel-major arrays of n
        const int n = clouds[k].n;
        const float* rec = reinterpret_cast<const float*>(host.data() + at);
        for (int i = 0; i < n; ++i) {
            const float* lo = rec + lo_off(i); const float* hi = rec + hi_off(n, i);
            xyz_out[3 * (size_t)i] = lo[0]; xyz_out[3 * (size_t)i + 1] = lo[1]; xyz_out[3 * (size_t)i + 2] = lo[2];
            feat_out[i] = lo[3]; feat_out[(size_t)n + i] = hi[0]; feat_out[2 * (size_t)n + i] = hi[1]; feat_out[3 * (size_t)n + i] = hi[2]; feat_out[4 * (size_t)n + i] = hi[3];
        }
        xyz_out += 3 * (size_t)n; feat_out += 5 * (size_t)n;
        at += (size_t)n * REC * sizeof(float);
        guard(at); at += G;
    }
    *guards_intact = ok;
    return CVO_OK;
}
// ---- reducing clouds (cvo_reduce_kernels.hip): a voxel-grid filter in front of the device-cloud hand-over.  The reducer holds one block of device
// scratch, cut per call into a region per cloud (a reduction) or per (cloud, voxel size) item (a count); nothing is allocated after creation.
// Fusing clouds (cvo_fuse_kernels.hip) runs groups of posed clouds through the same machinery, on the reducer's scratch and stream.  Reducing frames
// (cvo_hip.h, "Reducing frames") is the same launches with the frame as the point source: a FrameDesc per frame behind the call's records in the
// descriptor table, the records' cloud fields 0.  Viewing clouds (cvo_view_kernels.hip) uses the reducer's scratch, stream and counts for z-buffers.
struct cvo_reducer_s {
    int device = 0, max_clouds = 0, max_points = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    void* scratch = nullptr; size_t scratch_bytes = 0, cloud_bytes = 0;
    void* d_desc = nullptr; int* d_total = nullptr;                   // the launch's descriptor table and its row counts on the device
    void* h_desc = nullptr; int* h_total = nullptr;                   // their pinned twins: written before the launches, read after the call's one wait
    size_t table_bytes = 0;                                           // the size of d_desc and of h_desc
    int live_maps = 0;                                                // cvo_maps objects created on this reducer and not yet destroyed
    bool table_in_flight = false;                                     // a call without a host wait (CallEdges::may_return_early) left h_desc's copy queued
};
extern "C++" {                                                        // (the helpers below have templates among them)
namespace {
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
// a cloud's region of a reduction, laid out for the reducer's max_points (a call's cloud uses the front of each array)
struct ReduceLayout { size_t keys, sums, best, lowest, members, row, slot_of, block_heads, row_slot, bytes; };
ReduceLayout reduce_layout(int max_points) {
    const size_t P = (size_t)max_points, S = 2 * P, R = std::min<size_t>(P, 65535), B = (P + 255) / 256;
    ReduceLayout L; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    L.keys = take(8 * S); L.sums = take(64 * R); L.best = take(8 * R); L.lowest = take(4 * S); L.members = take(4 * S); L.row = take(4 * S);
    L.slot_of = take(4 * P); L.block_heads = take(4 * B); L.row_slot = take(4 * R); L.bytes = at;
    return L;
}
inline size_t count_item_keys(int n) { return up16(16 * (size_t)n); }                       // 2 n slots of 8 bytes
inline size_t count_item_bytes(int n) { return count_item_keys(n) + up16(8 * (size_t)n); }   // and their member counts
// A fusion: a group takes a cloud's region, and behind the max_clouds regions -- in the part of the 384 bytes per point that a reduction leaves
// unused -- its view masks (8 bytes per slot) and the heads of its blocks (a block per 256 points of a member: up to 64 more than a cloud of as
// many points has).  The descriptor table holds the groups' records, then the members'.
constexpr int FUSE_MAX_MEMBERS = 64, FUSE_MAX_CALL_MEMBERS = 4096;
inline size_t fuse_masks_bytes(int max_points) { return up16(16 * (size_t)max_points); }
inline size_t fuse_extra_bytes(int max_points) { return fuse_masks_bytes(max_points) + up16(4 * (((size_t)max_points + 255) / 256 + FUSE_MAX_MEMBERS)); }
inline size_t fuse_max_call_members(int max_clouds) { return std::min<size_t>(FUSE_MAX_CALL_MEMBERS, (size_t)max_clouds * FUSE_MAX_MEMBERS); }
inline size_t fuse_table_bytes(int max_clouds) { return (size_t)max_clouds * sizeof(FuseGroupDesc) + fuse_max_call_members(max_clouds) * sizeof(FuseMemberDesc); }
void reducer_release(cvo_reducer r) {
    (void)hipSetDevice(r->device);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->ev_in) (void)hipEventDestroy(r->ev_in);
    if (r->ev_out) (void)hipEventDestroy(r->ev_out);
    if (r->scratch) (void)hipFree(r->scratch);
    if (r->d_desc) (void)hipFree(r->d_desc);
    if (r->d_total) (void)hipFree(r->d_total);
    if (r->h_desc) (void)hipHostFree(r->h_desc);
    if (r->h_total) (void)hipHostFree(r->h_total);
    delete r;
}
int reducer_alloc(cvo_reducer r) {
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&r->ev_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&r->ev_out, hipEventDisableTiming));
    const size_t items = (size_t)r->max_clouds * CVO_REDUCE_MAX_VOXELS;
    r->cloud_bytes = reduce_layout(r->max_points).bytes;
    r->scratch_bytes = std::max((size_t)r->max_clouds * r->cloud_bytes, items * count_item_bytes(r->max_points));
    // the descriptor table of a call: its records, and for frames read in place (FrameDesc) one more record per frame behind them
    const size_t frames = (size_t)r->max_clouds * sizeof(FrameDesc);
    r->table_bytes = std::max({(size_t)r->max_clouds * sizeof(ReduceDesc) + frames, items * sizeof(CountDesc) + frames,
                               fuse_table_bytes(r->max_clouds) + fuse_max_call_members(r->max_clouds) * sizeof(FrameDesc),
                               frames + (size_t)r->max_clouds * sizeof(FrameCloudDst)});
    HIP_TRY(hipMalloc(&r->scratch, r->scratch_bytes));
    HIP_TRY(hipMalloc(&r->d_desc, r->table_bytes));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->d_total), items * sizeof(int)));
    HIP_TRY(hipHostMalloc(&r->h_desc, r->table_bytes, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&r->h_total), items * sizeof(int), hipHostMallocDefault));
    return CVO_OK;
}
// A call's descriptor table, carved record array by record array: the pinned array to fill and the device's copy of it at the same offset.
struct DescTable {
    cvo_reducer r; size_t used = 0;                                   // used: what the call copies to the device (reducer_run)
    template <class T> int take(size_t count, T** host, const T** dev) {
        if (r->table_in_flight) {                                     // (the pinned table is about to be written: its last copy must have left)
            HIP_TRY(hipEventSynchronize(r->ev_out));
            r->table_in_flight = false;
        }
        *host = reinterpret_cast<T*>(static_cast<char*>(r->h_desc) + used);
        *dev = reinterpret_cast<const T*>(static_cast<const char*>(r->d_desc) + used);
        used += sizeof(T) * count;
        if (used > r->table_bytes)                                    // (never: reducer_alloc sizes the table for the checked limits of every entry point)
            return fail(CVO_ERR_INVALID, "the reducer's descriptor table has no room for the call's " + std::to_string(used) + " bytes of records");
        return CVO_OK;
    }
};

// -- what the entry points check
// the input side of a reduction or a count of clouds: cvo_check_device_clouds' rules with the reducer's limits
int reduce_check_in(cvo_reducer r, int count, const cvo_device_cloud* in) {
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    if (count > r->max_clouds) return fail(CVO_ERR_INVALID, "count " + std::to_string(count) + " is above the reducer's max_clouds " + std::to_string(r->max_clouds));
    return check_device_clouds(r->device, count, in, r->max_points);   // (n above max_points: "cloud k: n ... is outside 0 .. max_points")
}
// the filter of a reduction or a fusion
int check_filter(float voxel, int mode, int min_points) {
    if (!(std::isfinite(voxel) && voxel > 0.f)) return fail(CVO_ERR_INVALID, "voxel " + std::to_string(voxel) + " is not a finite size above 0");
    if (mode != CVO_REDUCE_MEAN && mode != CVO_REDUCE_CENTRAL) return fail(CVO_ERR_INVALID, "mode " + std::to_string(mode) + " is neither CVO_REDUCE_MEAN nor CVO_REDUCE_CENTRAL");
    if (min_points < 1) return fail(CVO_ERR_INVALID, "min_points " + std::to_string(min_points) + " is below 1");
    return CVO_OK;
}
// the caller's arrays of one output (`who`: "cloud 3: "): aligned, and device memory to their last byte.  An array that is not required may be
// null, and one of no bytes (cap 0) is not looked at.
struct OutArray { const void* p; long long bytes; unsigned align; const char* name; bool required; };
int check_out_arrays(int device, const std::string& who, std::initializer_list<OutArray> arrays) {
    int rc;
    for (const OutArray& x : arrays) {
        if (!x.p && x.required) return fail(CVO_ERR_INVALID, who + x.name + " is null");
        if (!x.p || x.bytes == 0) continue;
        if (reinterpret_cast<uintptr_t>(x.p) & (x.align - 1u)) return fail(CVO_ERR_INVALID, who + x.name + " is not " + std::to_string(x.align) + "-byte aligned");
        if ((rc = check_device_plane(device, x.p, x.bytes, x.bytes, 1, who + x.name, "array"))) return rc;
    }
    return CVO_OK;
}
// the output side of a reduction (Dst: cvo_reduced_cloud) or a fusion (cvo_fused_cloud) of n points: the cap and the five arrays both have
template <class Dst>
int check_out_rows(int device, const std::string& who, const Dst& d, long long n, std::initializer_list<OutArray> more) {
    if (d.cap < 0 || d.cap > 65535) return fail(CVO_ERR_INVALID, who + "cap " + std::to_string(d.cap) + " is outside 0 .. 65535");
    if (d.cap > 0 && !d.xyz) return fail(CVO_ERR_INVALID, who + "dst xyz is null with cap " + std::to_string(d.cap));
    if (d.cap > 0 && !d.feat) return fail(CVO_ERR_INVALID, who + "dst feat is null with cap " + std::to_string(d.cap));
    int rc = check_out_arrays(device, who, {{d.xyz, 12ll * d.cap, 4, "dst xyz", false}, {d.feat, 20ll * d.cap, 4, "dst feat", false}, {d.count, 4ll * d.cap, 4, "dst count", false},
                                            {d.source, 4ll * d.cap, 4, "dst source", false}, {d.map, 4ll * n, 4, "dst map", false}});
    return rc ? rc : check_out_arrays(device, who, more);
}
// the parameters and the output side of a reduction of `count` clouds; n_of(k): cloud k's points (its map's entries)
int reduce_check_out(cvo_reducer r, int count, const std::function<int(int)>& n_of, const cvo_reduce_params* p, const cvo_reduced_cloud* dst) {
    int rc;
    if (!p || !dst) return fail(CVO_ERR_INVALID, "null argument");
    if ((rc = check_filter(p->voxel, p->mode, p->min_points))) return rc;
    for (int k = 0; k < count; ++k)
        if ((rc = check_out_rows(r->device, "cloud " + std::to_string(k) + ": ", dst[k], n_of(k), {}))) return rc;
    return CVO_OK;
}
int reduce_check(cvo_reducer r, int count, const cvo_device_cloud* in, const cvo_reduce_params* p, const cvo_reduced_cloud* dst) {
    int rc = reduce_check_in(r, count, in); if (rc) return rc;
    return reduce_check_out(r, count, [&](int k) { return in[k].n; }, p, dst);
}
int count_check_sizes(int k, const float* voxels, int min_points, const int* counts_out) {
    if (!voxels || !counts_out) return fail(CVO_ERR_INVALID, "null argument");
    if (k < 1 || k > CVO_REDUCE_MAX_VOXELS) return fail(CVO_ERR_INVALID, "k " + std::to_string(k) + " is outside 1 .. " + std::to_string(CVO_REDUCE_MAX_VOXELS));
    for (int j = 0; j < k; ++j)
        if (!(std::isfinite(voxels[j]) && voxels[j] > 0.f)) return fail(CVO_ERR_INVALID, "voxels[" + std::to_string(j) + "] " + std::to_string(voxels[j]) + " is not a finite size above 0");
    if (min_points < 1) return fail(CVO_ERR_INVALID, "min_points " + std::to_string(min_points) + " is below 1");
    return CVO_OK;
}
// the groups' shape and the filter of a fusion (members: the call's member array, looked at for null only)
int fuse_check_shape(cvo_reducer r, int groups, const int* group_first, const void* members, const cvo_fuse_params* p, const cvo_fused_cloud* dst) {
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    if (groups < 1 || groups > r->max_clouds) return fail(CVO_ERR_INVALID, "groups " + std::to_string(groups) + " is outside 1 .. the reducer's max_clouds " + std::to_string(r->max_clouds));
    if (!group_first || !members || !p || !dst) return fail(CVO_ERR_INVALID, "null argument");
    if (group_first[0] != 0) return fail(CVO_ERR_INVALID, "group_first[0] " + std::to_string(group_first[0]) + " is not 0");
    for (int g = 0; g < groups; ++g) {
        const long long k = (long long)group_first[g + 1] - group_first[g];
        if (k < 0) return fail(CVO_ERR_INVALID, "group_first[" + std::to_string(g + 1) + "] " + std::to_string(group_first[g + 1]) + " is below group_first[" + std::to_string(g) + "]: not ascending");
        if (k < 1 || k > FUSE_MAX_MEMBERS) return fail(CVO_ERR_INVALID, "group " + std::to_string(g) + ": " + std::to_string(k) + " members is outside 1 .. 64");
        if (group_first[g + 1] > FUSE_MAX_CALL_MEMBERS) return fail(CVO_ERR_INVALID, "group " + std::to_string(g) + ": more than 4096 members in the call");
    }
    if (int rc = check_filter(p->voxel, p->mode, p->min_points)) return rc;
    if (p->min_views < 1 || p->min_views > FUSE_MAX_MEMBERS) return fail(CVO_ERR_INVALID, "min_views " + std::to_string(p->min_views) + " is outside 1 .. 64");
    return CVO_OK;
}
int fuse_check_pose(const float* pose, const std::string& who) {
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose[k])) return fail(CVO_ERR_INVALID, who + "pose[" + std::to_string(k) + "] is not finite");
    return CVO_OK;
}
// the groups' sizes and the output side of a fusion; n_of(m): the points of member m of the call
int fuse_check_out(cvo_reducer r, int groups, const int* group_first, const std::function<long long(int)>& n_of, const cvo_fused_cloud* dst) {
    int rc;
    for (int g = 0; g < groups; ++g) {
        const std::string who = "group " + std::to_string(g) + ": ";
        long long n = 0;
        for (int m = group_first[g]; m < group_first[g + 1]; ++m) n += n_of(m);
        if (n > r->max_points) return fail(CVO_ERR_INVALID, who + "its members' " + std::to_string(n) + " points are above the reducer's max_points " + std::to_string(r->max_points));
        const cvo_fused_cloud& d = dst[g];
        if ((rc = check_out_rows(r->device, who, d, n, {{d.views, 4ll * d.cap, 4, "dst views", false}, {d.view_mask, 8ll * d.cap, 8, "dst view_mask", false}}))) return rc;
    }
    return CVO_OK;
}
int fuse_check(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_member* members, const cvo_fuse_params* p, const cvo_fused_cloud* dst) {
    int rc = fuse_check_shape(r, groups, group_first, members, p, dst); if (rc) return rc;
    const int total = group_first[groups];
    std::vector<cvo_device_cloud> clouds(total); std::vector<std::string> names(total);
    for (int g = 0; g < groups; ++g)
        for (int m = group_first[g]; m < group_first[g + 1]; ++m) {
            clouds[m] = members[m].cloud;
            names[m] = "group " + std::to_string(g) + " member " + std::to_string(m - group_first[g]) + ": ";
            if ((rc = fuse_check_pose(members[m].pose, names[m]))) return rc;
        }
    if ((rc = check_device_clouds(r->device, total, clouds.data(), r->max_points, names.data()))) return rc;
    return fuse_check_out(r, groups, group_first, [&](int m) { return (long long)members[m].cloud.n; }, dst);
}
int fuse_scratch_fits(cvo_reducer r) {
    if ((size_t)r->max_clouds * (r->cloud_bytes + fuse_extra_bytes(r->max_points)) > r->scratch_bytes)
        return fail(CVO_ERR_INVALID, "the reducer's scratch has no room for the view masks");   // (never: 136 of 384 bytes per point)
    return CVO_OK;
}
inline int frame_sub(int v, int step) { return (v + step - 1) / step; }
int frames_check_grid(cvo_reducer r, int width, int height, int step) {
    if (step < 1 || step > 16) return fail(CVO_ERR_INVALID, "step " + std::to_string(step) + " is outside 1 .. 16");
    const long long n = (long long)frame_sub(width, step) * frame_sub(height, step);
    if (n > r->max_points) return fail(CVO_ERR_INVALID, "a frame's " + std::to_string(n) + " points at step " + std::to_string(step) + " are above the reducer's max_points " + std::to_string(r->max_points));
    return CVO_OK;
}
int frames_check_camera(const cvo_camera* cams, int ci, const std::string& who) {
    if (ci < 0) return fail(CVO_ERR_INVALID, who + "camera index " + std::to_string(ci) + " is out of range");
    const cvo_camera& c = cams[ci];
    const struct { float v; const char* name; bool nonzero; } f[5] = {{c.scaling_factor, "scaling_factor", true}, {c.fx, "fx", true}, {c.fy, "fy", true}, {c.cx, "cx", false}, {c.cy, "cy", false}};
    for (const auto& x : f) {
        if (!std::isfinite(x.v)) return fail(CVO_ERR_INVALID, who + "camera " + std::to_string(ci) + ": " + x.name + " is not finite");
        if (x.nonzero && x.v == 0.f) return fail(CVO_ERR_INVALID, who + "camera " + std::to_string(ci) + ": " + x.name + " is 0");
    }
    return CVO_OK;
}
int frames_check(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams, const int* cam_index) {
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    int rc = check_device_images(r->device, count, images, width, height); if (rc) return rc;
    if (count > r->max_clouds) return fail(CVO_ERR_INVALID, "count " + std::to_string(count) + " is above the reducer's max_clouds " + std::to_string(r->max_clouds));
    if ((rc = frames_check_grid(r, width, height, step))) return rc;
    if (!cams) return fail(CVO_ERR_INVALID, "null argument: cams");
    for (int k = 0; k < count; ++k)
        if ((rc = frames_check_camera(cams, cam_index ? cam_index[k] : 0, "frame " + std::to_string(k) + ": "))) return rc;
    return CVO_OK;
}
int fuse_frames_check(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                      const cvo_fuse_params* p, const cvo_fused_cloud* dst) {
    int rc = fuse_check_shape(r, groups, group_first, members, p, dst); if (rc) return rc;
    const int total = group_first[groups];
    std::vector<cvo_device_image> images(total);
    for (int m = 0; m < total; ++m) images[m] = members[m].image;
    if ((rc = check_device_images(r->device, total, images.data(), width, height))) return rc;   // ("image m": the member's place in the call)
    if ((rc = frames_check_grid(r, width, height, step))) return rc;
    if (!cams) return fail(CVO_ERR_INVALID, "null argument: cams");
    for (int g = 0; g < groups; ++g)
        for (int m = group_first[g]; m < group_first[g + 1]; ++m) {
            const std::string who = "group " + std::to_string(g) + " member " + std::to_string(m - group_first[g]) + ": ";
            if ((rc = fuse_check_pose(members[m].pose, who)) || (rc = frames_check_camera(cams, members[m].cam, who))) return rc;
        }
    const long long n = (long long)frame_sub(width, step) * frame_sub(height, step);
    return fuse_check_out(r, groups, group_first, [&](int) { return n; }, dst);
}

// -- what the entry points write into their records
// a record's point source: a cloud's arrays with the strides resolved, or 0 in all five fields -- a frame read in place (its FrameDesc says where)
template <class Rec>
void set_cloud_source(Rec& D, const cvo_device_cloud* c) {
    D.xyz = c ? static_cast<const float*>(c->xyz) : nullptr; D.feat = c ? static_cast<const float*>(c->feat) : nullptr;
    D.xyz_stride = D.feat_point_stride = D.feat_channel_stride = 0;
    if (c) cloud_strides(*c, &D.xyz_stride, &D.feat_point_stride, &D.feat_channel_stride);
}
void frame_desc(const cvo_device_image& im, int w, int h, int step, const cvo_camera& c, FrameDesc& F) {
    F.bgr = static_cast<const uint8_t*>(im.bgr8); F.depth = static_cast<const uint8_t*>(im.depth16);
    F.bgr_pitch = im.bgr_pitch ? im.bgr_pitch : (long long)w * im.pixel_bytes;
    F.depth_pitch = im.depth_pitch ? im.depth_pitch : 2ll * w;
    F.pixel_bytes = im.pixel_bytes; F.swap_rb = im.swap_rb;
    F.w = w; F.h = h; F.step = step; F.ws = frame_sub(w, step);
    F.scaling_factor = c.scaling_factor; F.fx = c.fx; F.fy = c.fy; F.cx = c.cx; F.cy = c.cy; F.pad_ = 0;
}
// Where the points of a call's items come from (a reduction's or a count's clouds, a fusion's members): device clouds, or frames read in place,
// all of frame_n > 0 points and each with a FrameDesc row behind the records
struct PointSource {
    std::function<const cvo_device_cloud*(int)> cloud;                // item k's cloud; unset: the items are frames
    std::function<void(int, FrameDesc&)> frame;                       // item k's frame row
    int frame_n = 0;
    bool frames() const { return !cloud; }
    int n(int k) const { return cloud ? cloud(k)->n : frame_n; }
    template <class Rec> void fill(int k, Rec& D, FrameDesc* rows, int at) const {   // rows[at]: the row of D's frame (not looked at with clouds)
        set_cloud_source(D, cloud ? cloud(k) : nullptr);
        if (!cloud) frame(k, rows[at]);
    }
};
PointSource frames_source(const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams, const int* cam_index) {
    PointSource src;
    src.frame = [=](int k, FrameDesc& F) { frame_desc(images[k], width, height, step, cams[cam_index ? cam_index[k] : 0], F); };
    src.frame_n = frame_sub(width, step) * frame_sub(height, step);
    return src;
}
// region q of the scratch and the output arrays of d (a cvo_reduced_cloud or a cvo_fused_cloud, of n points) in record D
template <class Rec, class Dst>
void desc_scratch_out(cvo_reducer r, const ReduceLayout& L, int q, const Dst& d, int n, Rec& D) {
    char* base = static_cast<char*>(r->scratch) + (size_t)q * r->cloud_bytes;
    D.keys = reinterpret_cast<unsigned long long*>(base + L.keys); D.lowest = reinterpret_cast<unsigned*>(base + L.lowest);
    D.members = reinterpret_cast<unsigned*>(base + L.members); D.row = reinterpret_cast<int*>(base + L.row);
    D.slot_of = reinterpret_cast<int*>(base + L.slot_of); D.block_heads = reinterpret_cast<int*>(base + L.block_heads);
    D.row_slot = reinterpret_cast<int*>(base + L.row_slot); D.sums = reinterpret_cast<long long*>(base + L.sums);
    D.best = reinterpret_cast<unsigned long long*>(base + L.best);
    D.out_xyz = static_cast<float*>(d.xyz); D.out_feat = static_cast<float*>(d.feat); D.out_count = static_cast<int*>(d.count);
    D.out_source = static_cast<int*>(d.source); D.out_map = static_cast<int*>(d.map);
    D.total = r->d_total + q;
    D.n = n; D.slots = 2 * n; D.cap = d.cap; D.rows_cap = std::min(d.cap, n);
}
// The edges of every call on the reducer's stream, written once: the reducer's stream behind the caller's, the call's tables to the device, its
// figures zeroed, the launches (queue), the figures to pinned memory, the caller's stream behind the reducer's, and the call's one host wait --
// or none: a call with a stream and nothing to read back may return with its table's copy still queued, which the next DescTable::take settles.
struct CallEdges {
    const char* name;                                                 // of the kernels, for the launch-failure message
    size_t table_bytes = 0;                                           // of the reducer's descriptor table (0: none)
    const void* own_host = nullptr; void* own_dev = nullptr; size_t own_bytes = 0;   // a table of the caller's own copied beside it (a maps object's MapDescs)
    int zero_figures = 0, read_figures = 0;                           // ints of the reducer's counts zeroed first / copied to h_total behind the launches
    bool may_return_early = false;
};
int run_call(cvo_reducer r, const CallEdges& c, void* stream, const std::function<hipError_t()>& queue) {
    hipStream_t cs = static_cast<hipStream_t>(stream);
    if (cs) { HIP_TRY(hipEventRecord(r->ev_in, cs)); HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_in, 0)); }
    if (c.table_bytes) HIP_TRY(hipMemcpyAsync(r->d_desc, r->h_desc, c.table_bytes, hipMemcpyHostToDevice, r->stream));
    if (c.own_bytes) HIP_TRY(hipMemcpyAsync(c.own_dev, c.own_host, c.own_bytes, hipMemcpyHostToDevice, r->stream));
    if (c.zero_figures > 0) HIP_TRY(hipMemsetAsync(r->d_total, 0, sizeof(int) * (size_t)c.zero_figures, r->stream));
    const hipError_t e = queue();
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string(c.name) + " kernel launch: " + hipGetErrorString(e));
    if (c.read_figures > 0) HIP_TRY(hipMemcpyAsync(r->h_total, r->d_total, sizeof(int) * (size_t)c.read_figures, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipEventRecord(r->ev_out, r->stream));
    if (cs) HIP_TRY(hipStreamWaitEvent(cs, r->ev_out, 0));
    if (c.may_return_early && cs && c.read_figures == 0) { r->table_in_flight = true; return CVO_OK; }   // (the outputs are ordered on the caller's stream)
    HIP_TRY(hipEventSynchronize(r->ev_out));                          // (the call's one host wait)
    return CVO_OK;
}
int reducer_run(cvo_reducer r, size_t table_bytes, int n_totals, void* cloud_stream, const std::function<hipError_t()>& queue) {
    CallEdges c{"cloud reduce"};
    c.table_bytes = table_bytes; c.read_figures = n_totals;
    return run_call(r, c, cloud_stream, queue);
}

// -- reduce, count and fuse, each once over a point source: the checked call's items with points (a frame always has some) get records, in order
int reduce_points(cvo_reducer r, int count, const PointSource& src, const cvo_reduce_params* p, const cvo_reduced_cloud* dst, int* n_out, void* stream) {
    if (!n_out) return fail(CVO_ERR_INVALID, "null argument: n_out");
    HIP_TRY(hipSetDevice(r->device));
    const ReduceLayout L = reduce_layout(r->max_points);
    std::vector<int> of; of.reserve(count);
    for (int k = 0; k < count; ++k) { n_out[k] = 0; if (src.n(k) > 0) of.push_back(k); }
    const int live = (int)of.size();
    if (live == 0) return CVO_OK;
    DescTable tab{r};
    ReduceDesc* h; const ReduceDesc* d; FrameDesc* hf = nullptr; const FrameDesc* df = nullptr;
    int rc = tab.take(live, &h, &d); if (rc) return rc;
    if (src.frames() && (rc = tab.take(live, &hf, &df))) return rc;
    int n_max = 0, rows_max = 0;
    for (int q = 0; q < live; ++q) {
        const int k = of[q], n = src.n(k);
        src.fill(k, h[q], hf, q);
        desc_scratch_out(r, L, q, dst[k], n, h[q]);
        n_max = std::max(n_max, n); rows_max = std::max(rows_max, h[q].rows_cap);
    }
    const cvo_reduce_params P = *p;
    if ((rc = reducer_run(r, tab.used, live, stream, [&] {
            return src.frames() ? launch_reduce_frames(d, df, live, n_max, rows_max, P.voxel, P.mode, P.min_points, r->stream)
                                : launch_reduce_clouds(d, live, n_max, 2 * n_max, rows_max, P.voxel, P.mode, P.min_points, r->stream); })))
        return rc;
    for (int q = 0; q < live; ++q) n_out[of[q]] = r->h_total[q];
    return CVO_OK;
}
// item (i, j) is source i at voxels[j]: a table of its own, one after the other in the scratch
int count_points(cvo_reducer r, int count, const PointSource& src, int k, const float* voxels, int min_points, int* counts_out, void* stream) {
    HIP_TRY(hipSetDevice(r->device));
    std::vector<int> of; of.reserve(count);
    for (int i = 0; i < count; ++i) {
        for (int j = 0; j < k; ++j) counts_out[i * k + j] = 0;
        if (src.n(i) > 0) of.push_back(i);
    }
    const int sources = (int)of.size(), live = sources * k;
    if (live == 0) return CVO_OK;
    DescTable tab{r};
    CountDesc* h; const CountDesc* d; FrameDesc* hf = nullptr; const FrameDesc* df = nullptr;
    int rc = tab.take(live, &h, &d); if (rc) return rc;
    if (src.frames() && (rc = tab.take(sources, &hf, &df))) return rc;
    size_t at = 0; int n_max = 0;
    for (int f = 0; f < sources; ++f) {
        const int i = of[f], n = src.n(i);
        for (int j = 0; j < k; ++j) {
            const int q = f * k + j;
            char* base = static_cast<char*>(r->scratch) + at; at += count_item_bytes(n);   // (at most max_clouds x 16 items of max_points: inside the scratch)
            CountDesc& D = h[q];
            src.fill(i, D, hf, f);
            D.keys = reinterpret_cast<unsigned long long*>(base); D.members = reinterpret_cast<unsigned*>(base + count_item_keys(n));
            D.total = r->d_total + q; D.n = n; D.slots = 2 * n; D.voxel = voxels[j]; D.src = src.frames() ? f : 0;
        }
        n_max = std::max(n_max, n);
    }
    if ((rc = reducer_run(r, tab.used, live, stream, [&] {
            return src.frames() ? launch_count_frame_voxels(d, df, live, n_max, min_points, r->stream)
                                : launch_count_voxels(d, live, n_max, 2 * n_max, min_points, r->stream); })))
        return rc;
    for (int q = 0; q < live; ++q) counts_out[of[q / k] * k + q % k] = r->h_total[q];
    return CVO_OK;
}
// src's item m is member m of the call, pose(m) its 12 floats; a group with points gets a record, and behind the groups' records its members with points
int fuse_points(cvo_reducer r, int groups, const int* group_first, const PointSource& src, const std::function<const float*(int)>& pose, const cvo_fuse_params* p,
                const cvo_fused_cloud* dst, int* n_out, void* stream) {
    if (!n_out) return fail(CVO_ERR_INVALID, "null argument: n_out");
    int rc = fuse_scratch_fits(r); if (rc) return rc;
    HIP_TRY(hipSetDevice(r->device));
    const ReduceLayout L = reduce_layout(r->max_points);
    std::vector<int> of; of.reserve(groups);
    int live_members = 0;
    for (int g = 0; g < groups; ++g) {
        n_out[g] = 0;
        const int before = live_members;
        for (int m = group_first[g]; m < group_first[g + 1]; ++m) live_members += src.n(m) > 0;
        if (live_members > before) of.push_back(g);
    }
    const int live_groups = (int)of.size();
    if (live_groups == 0) return CVO_OK;
    DescTable tab{r};
    FuseGroupDesc* hg; const FuseGroupDesc* dg; FuseMemberDesc* hm; const FuseMemberDesc* dm; FrameDesc* hf = nullptr; const FrameDesc* df = nullptr;
    if ((rc = tab.take(live_groups, &hg, &dg)) || (rc = tab.take(live_members, &hm, &dm))) return rc;
    if (src.frames() && (rc = tab.take(live_members, &hf, &df))) return rc;
    const size_t extra = fuse_extra_bytes(r->max_points), extras_at = (size_t)r->max_clouds * r->cloud_bytes;
    int n_max = 0, slots_max = 0, rows_max = 0, qm = 0;
    for (int q = 0; q < live_groups; ++q) {
        const int g = of[q];
        FuseGroupDesc& G = hg[q];
        G.first_member = qm;
        int at = 0, blocks = 0;
        for (int m = group_first[g]; m < group_first[g + 1]; ++m) {
            const int n = src.n(m);
            if (n == 0) continue;
            FuseMemberDesc& M = hm[qm];
            src.fill(m, M, hf, qm);
            ++qm;
            std::memcpy(M.pose, pose(m), sizeof(M.pose));
            M.group = q; M.base = at; M.first_block = blocks; M.n = n; M.bit = m - group_first[g]; M.pad_ = 0;
            at += n; blocks += (n + 255) / 256;
            n_max = std::max(n_max, n);
        }
        desc_scratch_out(r, L, q, dst[g], at, G);
        char* more = static_cast<char*>(r->scratch) + extras_at + (size_t)q * extra;   // the group's masks and block heads: behind the regions
        G.masks = reinterpret_cast<unsigned long long*>(more); G.block_heads = reinterpret_cast<int*>(more + fuse_masks_bytes(r->max_points));
        G.out_views = static_cast<int*>(dst[g].views); G.out_view_mask = static_cast<unsigned long long*>(dst[g].view_mask);
        G.n_blocks = blocks; G.n_members = qm - G.first_member; G.pad_ = 0;
        slots_max = std::max(slots_max, G.slots); rows_max = std::max(rows_max, G.rows_cap);
    }
    const cvo_fuse_params P = *p;
    if ((rc = reducer_run(r, tab.used, live_groups, stream, [&] {
            return src.frames() ? launch_fuse_frames(dg, live_groups, dm, df, live_members, n_max, slots_max, rows_max, P.voxel, P.mode, P.min_points, P.min_views, r->stream)
                                : launch_fuse_clouds(dg, live_groups, dm, live_members, n_max, slots_max, rows_max, P.voxel, P.mode, P.min_points, P.min_views, r->stream); })))
        return rc;
    for (int q = 0; q < live_groups; ++q) n_out[of[q]] = r->h_total[q];
    return CVO_OK;
}

// -- viewing clouds (cvo_view_kernels.hip; cvo_hip.h, "Viewing clouds").  View q takes region q of the scratch -- its z-buffer, its points' code
// words, its blocks' counts and their relation counts, laid out for max_points -- and five of the reducer's counts: its rows, then its four
// relation counts.
struct ViewLayout { size_t code, block_heads, block_relations, bytes; };   // (the z-buffer is at 0)
ViewLayout view_layout(int max_points) {
    const size_t P = (size_t)max_points;
    ViewLayout L;
    const size_t B = (P + 255) / 256;
    L.code = up16(8 * P); L.block_heads = L.code + up16(4 * P); L.block_relations = L.block_heads + up16(4 * B); L.bytes = L.block_relations + up16(16 * B);
    return L;
}
constexpr int VIEW_COUNTS = 5;
int view_check_params(cvo_reducer r, const cvo_view_params& p) {
    const struct { int v; const char* name; } sizes[2] = {{p.width, "width"}, {p.height, "height"}};
    for (const auto& s : sizes)
        if (s.v < 1 || s.v > 8192) return fail(CVO_ERR_INVALID, std::string(s.name) + " " + std::to_string(s.v) + " is outside 1 .. 8192");
    if (p.cell < 1 || p.cell > 16) return fail(CVO_ERR_INVALID, "cell " + std::to_string(p.cell) + " is outside 1 .. 16");
    if (p.mode != CVO_VIEW_FRONT && p.mode != CVO_VIEW_SURFACE) return fail(CVO_ERR_INVALID, "mode " + std::to_string(p.mode) + " is neither CVO_VIEW_FRONT nor CVO_VIEW_SURFACE");
    if (!(std::isfinite(p.z_near) && p.z_near > 0.f)) return fail(CVO_ERR_INVALID, "z_near " + std::to_string(p.z_near) + " is not a finite depth above 0");
    if (!(std::isfinite(p.z_far) && p.z_far > p.z_near && p.z_far <= 32768.f))
        return fail(CVO_ERR_INVALID, "z_far " + std::to_string(p.z_far) + " is not a finite depth above z_near " + std::to_string(p.z_near) + " and at most 32768");
    if (!(std::isfinite(p.slack) && p.slack >= 0.f)) return fail(CVO_ERR_INVALID, "slack " + std::to_string(p.slack) + " is not finite and at least 0");
    if (!(std::isfinite(p.depth_tol) && p.depth_tol >= 0.f)) return fail(CVO_ERR_INVALID, "depth_tol " + std::to_string(p.depth_tol) + " is not finite and at least 0");
    const long long cells = (long long)frame_sub(p.width, p.cell) * frame_sub(p.height, p.cell);
    if (cells > r->max_points) return fail(CVO_ERR_INVALID, "the " + std::to_string(cells) + " z-cells of " + std::to_string(p.width) + " x " + std::to_string(p.height) + " at cell " +
                                           std::to_string(p.cell) + " are above the reducer's max_points " + std::to_string(r->max_points));
    return CVO_OK;
}
// the depth plane of a view's observed image: cvo_check_device_images' rules for that plane alone (the colour fields are not looked at)
int view_check_observed(int device, const cvo_device_image& im, int width, int height, const std::string& who) {
    const long long drow = 2ll * width;
    if (!im.depth16) return fail(CVO_ERR_INVALID, who + "observed depth16 is null");
    if (im.depth_pitch < 0 || (im.depth_pitch != 0 && im.depth_pitch < drow)) return fail(CVO_ERR_INVALID, who + "observed depth_pitch " + std::to_string(im.depth_pitch) + " is below the row's " + std::to_string(drow) + " bytes");
    if (reinterpret_cast<uintptr_t>(im.depth16) & 1u) return fail(CVO_ERR_INVALID, who + "observed depth16 is not 2-byte aligned");
    if (im.depth_pitch & 1) return fail(CVO_ERR_INVALID, who + "observed depth_pitch is not a multiple of 2");
    return check_device_plane(device, im.depth16, im.depth_pitch ? im.depth_pitch : drow, drow, height, who + "observed depth16");
}
int view_check(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
               const cvo_viewed_cloud* dst) {
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    if (views < 1 || views > r->max_clouds) return fail(CVO_ERR_INVALID, "views " + std::to_string(views) + " is outside 1 .. the reducer's max_clouds " + std::to_string(r->max_clouds));
    if (!v || !cams || !p || !dst) return fail(CVO_ERR_INVALID, "null argument");
    int rc = view_check_params(r, *p); if (rc) return rc;
    if (view_layout(r->max_points).bytes > r->cloud_bytes) return fail(CVO_ERR_INVALID, "the reducer's scratch has no room for a view");   // (never: under 13 of 384 bytes per point)
    std::vector<cvo_device_cloud> clouds(views); std::vector<std::string> names(views);
    for (int k = 0; k < views; ++k) {
        clouds[k] = v[k].cloud; names[k] = "view " + std::to_string(k) + ": ";
        if ((rc = fuse_check_pose(v[k].pose, names[k])) || (rc = frames_check_camera(cams, v[k].cam, names[k]))) return rc;
    }
    if ((rc = check_device_clouds(r->device, views, clouds.data(), r->max_points, names.data()))) return rc;
    const long long cells = (long long)frame_sub(p->width, p->cell) * frame_sub(p->height, p->cell);
    for (int k = 0; k < views; ++k) {
        const cvo_viewed_cloud& d = dst[k];
        const std::string& who = names[k];
        if (d.cap < 0 || d.cap > 65535) return fail(CVO_ERR_INVALID, who + "cap " + std::to_string(d.cap) + " is outside 0 .. 65535");
        if (d.cap > 0 && !d.xyz) return fail(CVO_ERR_INVALID, who + "dst xyz is null with cap " + std::to_string(d.cap));
        if (d.cap > 0 && !d.feat) return fail(CVO_ERR_INVALID, who + "dst feat is null with cap " + std::to_string(d.cap));
        if (d.relation && !observed) return fail(CVO_ERR_INVALID, who + "dst relation is set but observed is null");
        if (observed && (rc = view_check_observed(r->device, observed[k], p->width, p->height, who))) return rc;
        if ((rc = check_out_arrays(r->device, who, {{d.xyz, 12ll * d.cap, 4, "dst xyz", false}, {d.feat, 20ll * d.cap, 4, "dst feat", false},
                                                    {d.source, 4ll * d.cap, 4, "dst source", false}, {d.pixel, 4ll * d.cap, 4, "dst pixel", false},
                                                    {d.relation, 4ll * d.cap, 4, "dst relation", false}, {d.map, 4ll * v[k].cloud.n, 4, "dst map", false},
                                                    {d.depth, 4 * cells, 4, "dst depth", false}, {d.index, 4 * cells, 4, "dst index", false}}))) return rc;
    }
    return CVO_OK;
}
// every view gets a record, an empty cloud too: its depth and index images are written all the same
int view_points(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                const cvo_viewed_cloud* dst, int* n_out, int* relation_counts, void* stream) {
    if (!n_out) return fail(CVO_ERR_INVALID, "null argument: n_out");
    HIP_TRY(hipSetDevice(r->device));
    const ViewLayout L = view_layout(r->max_points);
    DescTable tab{r};
    ViewDesc* h; const ViewDesc* d;
    int rc = tab.take(views, &h, &d); if (rc) return rc;
    ViewParams P;
    P.width = p->width; P.height = p->height; P.cell = p->cell; P.mode = p->mode; P.gw = frame_sub(p->width, p->cell); P.gh = frame_sub(p->height, p->cell);
    P.z_near = p->z_near; P.z_far = p->z_far; P.slack = p->slack; P.depth_tol = p->depth_tol;
    int n_max = 0; bool images = false;
    for (int q = 0; q < views; ++q) {
        ViewDesc& V = h[q];
        const cvo_camera& c = cams[v[q].cam];
        set_cloud_source(V, &v[q].cloud);
        std::memcpy(V.pose, v[q].pose, sizeof(V.pose));
        V.fx = c.fx; V.fy = c.fy; V.cx = c.cx; V.cy = c.cy; V.scaling_factor = c.scaling_factor; V.n = v[q].cloud.n;
        char* base = static_cast<char*>(r->scratch) + (size_t)q * r->cloud_bytes;
        V.zbuf = reinterpret_cast<unsigned long long*>(base); V.code = reinterpret_cast<int*>(base + L.code); V.block_heads = reinterpret_cast<int*>(base + L.block_heads);
        V.block_relations = reinterpret_cast<int*>(base + L.block_relations);
        V.total = r->d_total + VIEW_COUNTS * q; V.relation_counts = V.total + 1;
        V.observed = observed ? static_cast<const uint8_t*>(observed[q].depth16) : nullptr;
        V.observed_pitch = observed && observed[q].depth_pitch ? observed[q].depth_pitch : 2ll * p->width;
        const cvo_viewed_cloud& o = dst[q];
        V.out_xyz = static_cast<float*>(o.xyz); V.out_feat = static_cast<float*>(o.feat); V.out_source = static_cast<int*>(o.source);
        V.out_pixel = static_cast<int*>(o.pixel); V.out_relation = static_cast<int*>(o.relation); V.out_map = static_cast<int*>(o.map);
        V.out_depth = static_cast<float*>(o.depth); V.out_index = static_cast<int*>(o.index);
        V.cap = o.cap; V.pad_ = 0;
        n_max = std::max(n_max, V.n); images = images || o.depth || o.index;
    }
    if ((rc = reducer_run(r, tab.used, VIEW_COUNTS * views, stream, [&] { return launch_view_clouds(d, views, n_max, P, observed != nullptr, images, r->stream); }))) return rc;
    for (int q = 0; q < views; ++q) {
        n_out[q] = r->h_total[VIEW_COUNTS * q];
        if (relation_counts)
            for (int k = 0; k < 4; ++k) relation_counts[4 * q + k] = observed ? r->h_total[VIEW_COUNTS * q + 1 + k] : 0;
    }
    return CVO_OK;
}
}  // namespace
}  // extern "C++"
int cvo_reducer_create(int device, int max_clouds, int max_points, cvo_reducer* out) {
    if (!out) return fail(CVO_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_clouds < 1 || max_clouds > 4095) return fail(CVO_ERR_INVALID, "max_clouds " + std::to_string(max_clouds) + " is outside 1 .. 4095");
    if (max_points < 1 || max_points > CVO_REDUCE_MAX_POINTS) return fail(CVO_ERR_INVALID, "max_points " + std::to_string(max_points) + " is outside 1 .. " + std::to_string(CVO_REDUCE_MAX_POINTS));
    int rc = check_device(device, nullptr); if (rc) return rc;
    cvo_reducer r = new cvo_reducer_s();
    r->device = device; r->max_clouds = max_clouds; r->max_points = max_points;
    if ((rc = reducer_alloc(r))) { reducer_release(r); return rc; }
    *out = r;
    return CVO_OK;
}
int cvo_reducer_destroy(cvo_reducer r) {
    if (r && r->live_maps > 0)
        return fail(CVO_ERR_INVALID, std::to_string(r->live_maps) + " cvo_maps object(s) still live on this reducer: destroy the maps first");
    if (r) reducer_release(r);
    return CVO_OK;
}
int cvo_reducer_info(cvo_reducer r, int* max_clouds, int* max_points, long long* scratch_bytes) {
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    if (max_clouds) *max_clouds = r->max_clouds;
    if (max_points) *max_points = r->max_points;
    if (scratch_bytes) *scratch_bytes = (long long)r->scratch_bytes;
    return CVO_OK;
}
int cvo_check_reduce_clouds(cvo_reducer r, int count, const cvo_device_cloud* in, const cvo_reduce_params* p, const cvo_reduced_cloud* dst) {
    return reduce_check(r, count, in, p, dst);
}
int cvo_reduce_device_clouds(cvo_reducer r, int count, const cvo_device_cloud* in, const cvo_reduce_params* p, const cvo_reduced_cloud* dst, int* n_out,
                             void* cloud_stream) {
    int rc = reduce_check(r, count, in, p, dst); if (rc) return rc;
    PointSource src; src.cloud = [&](int k) { return &in[k]; };
    return reduce_points(r, count, src, p, dst, n_out, cloud_stream);
}
int cvo_count_voxels(cvo_reducer r, int count, const cvo_device_cloud* in, int k, const float* voxels, int min_points, int* counts_out, void* cloud_stream) {
    int rc = reduce_check_in(r, count, in); if (rc) return rc;
    if ((rc = count_check_sizes(k, voxels, min_points, counts_out))) return rc;
    PointSource src; src.cloud = [&](int i) { return &in[i]; };
    return count_points(r, count, src, k, voxels, min_points, counts_out, cloud_stream);
}
int cvo_check_fuse_clouds(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_member* members, const cvo_fuse_params* p, const cvo_fused_cloud* dst) {
    return fuse_check(r, groups, group_first, members, p, dst);
}
int cvo_fuse_device_clouds(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_member* members, const cvo_fuse_params* p, const cvo_fused_cloud* dst,
                           int* n_out, void* cloud_stream) {
    int rc = fuse_check(r, groups, group_first, members, p, dst); if (rc) return rc;
    PointSource src; src.cloud = [&](int m) { return &members[m].cloud; };
    return fuse_points(r, groups, group_first, src, [&](int m) { return members[m].pose; }, p, dst, n_out, cloud_stream);
}
int cvo_check_device_frames(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams, const int* cam_index) {
    return frames_check(r, count, images, width, height, step, cams, cam_index);
}
int cvo_frames_to_device_clouds(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                                const int* cam_index, const cvo_frame_cloud* dst, void* image_stream) {
    int rc = frames_check(r, count, images, width, height, step, cams, cam_index); if (rc) return rc;
    if (!dst) return fail(CVO_ERR_INVALID, "null argument: dst");
    const PointSource src = frames_source(images, width, height, step, cams, cam_index);
    const int n = src.frame_n;
    for (int k = 0; k < count; ++k)
        if ((rc = check_out_arrays(r->device, "frame " + std::to_string(k) + ": ", {{dst[k].xyz, 12ll * n, 4, "dst xyz", true}, {dst[k].feat, 20ll * n, 4, "dst feat", true}}))) return rc;
    HIP_TRY(hipSetDevice(r->device));
    DescTable tab{r};
    FrameDesc* hf; const FrameDesc* df; FrameCloudDst* hd; const FrameCloudDst* dd;
    if ((rc = tab.take(count, &hf, &df)) || (rc = tab.take(count, &hd, &dd))) return rc;
    for (int k = 0; k < count; ++k) {
        src.frame(k, hf[k]);
        hd[k].xyz = static_cast<float*>(dst[k].xyz); hd[k].feat = static_cast<float*>(dst[k].feat);
    }
    return reducer_run(r, tab.used, 0, image_stream, [&] { return launch_frames_to_clouds(df, dd, count, n, r->stream); });
}
int cvo_reduce_device_frames(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                             const int* cam_index, const cvo_reduce_params* p, const cvo_reduced_cloud* dst, int* n_out, void* image_stream) {
    int rc = frames_check(r, count, images, width, height, step, cams, cam_index); if (rc) return rc;
    const PointSource src = frames_source(images, width, height, step, cams, cam_index);
    if ((rc = reduce_check_out(r, count, [&](int) { return src.frame_n; }, p, dst))) return rc;
    return reduce_points(r, count, src, p, dst, n_out, image_stream);
}
int cvo_count_frame_voxels(cvo_reducer r, int count, const cvo_device_image* images, int width, int height, int step, const cvo_camera* cams,
                           const int* cam_index, int k, const float* voxels, int min_points, int* counts_out, void* image_stream) {
    int rc = frames_check(r, count, images, width, height, step, cams, cam_index); if (rc) return rc;
    if ((rc = count_check_sizes(k, voxels, min_points, counts_out))) return rc;
    return count_points(r, count, frames_source(images, width, height, step, cams, cam_index), k, voxels, min_points, counts_out, image_stream);
}
int cvo_check_fuse_frames(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                          const cvo_fuse_params* p, const cvo_fused_cloud* dst) {
    return fuse_frames_check(r, groups, group_first, members, width, height, step, cams, p, dst);
}
int cvo_fuse_device_frames(cvo_reducer r, int groups, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                           const cvo_fuse_params* p, const cvo_fused_cloud* dst, int* n_out, void* image_stream) {
    int rc = fuse_frames_check(r, groups, group_first, members, width, height, step, cams, p, dst); if (rc) return rc;
    PointSource src;
    src.frame = [&](int m, FrameDesc& F) { frame_desc(members[m].image, width, height, step, cams[members[m].cam], F); };
    src.frame_n = frame_sub(width, step) * frame_sub(height, step);
    return fuse_points(r, groups, group_first, src, [&](int m) { return members[m].pose; }, p, dst, n_out, image_stream);
}
int cvo_check_view_clouds(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                          const cvo_viewed_cloud* dst) {
    return view_check(r, views, v, cams, p, observed, dst);
}
int cvo_view_device_clouds(cvo_reducer r, int views, const cvo_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                           const cvo_viewed_cloud* dst, int* n_out, int* relation_counts, void* cloud_stream) {
    int rc = view_check(r, views, v, cams, p, observed, dst); if (rc) return rc;
    return view_points(r, views, v, cams, p, observed, dst, n_out, relation_counts, cloud_stream);
}
// ---- resident maps (cvo_map_kernels.hip; cvo_hip.h, "Resident maps"): voxel maps that stay on the device between calls.  The object owns the
// maps' rows (twice: a compaction moves them to the other side), their tables and block counts, and a descriptor table of its own (a MapDesc per
// map of a call); an update's fusion passes run in the reducer's scratch, a group per region of map_layout, with the reducer's descriptor table,
// counts and stream.  A call's figures are four ints per map of the call in the reducer's counts.
struct cvo_maps_s {
    cvo_reducer r = nullptr;
    int max_maps = 0, max_rows = 0; float voxel = 0.f;
    char* mem = nullptr; size_t bytes = 0, map_bytes = 0;             // all maps' device memory, a map's share
    int* d_live = nullptr;                                            // max_maps ints at the front of mem
    MapDesc* d_desc = nullptr; MapDesc* h_desc = nullptr;             // max_maps records: the device's and the pinned twin
    std::vector<int> rows; std::vector<char> side;                    // per map: its rows (dead ones included), which side holds them
};
extern "C++" {
namespace {
constexpr int MAP_FIGURES = 4;                                        // per map of a call: cells or rows out, births, refusal bits, unused
// a group's region of the scratch in an update: a fusion's arrays with one row per point (the cap is the group's points), and cell_row
struct MapLayout { size_t keys, masks, sums, best, lowest, members, row, slot_of, row_slot, cell_row, block_heads, bytes; };
MapLayout map_layout(int max_points) {
    const size_t P = (size_t)max_points, S = 2 * P, B = (P + 255) / 256 + FUSE_MAX_MEMBERS;
    MapLayout L; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    L.keys = take(8 * S); L.masks = take(8 * S); L.sums = take(64 * P); L.best = take(8 * P); L.lowest = take(4 * S); L.members = take(4 * S);
    L.row = take(4 * S); L.slot_of = take(4 * P); L.row_slot = take(4 * P); L.cell_row = take(4 * P); L.block_heads = take(4 * B); L.bytes = at;
    return L;
}
// a map's share of the object's memory: two sides of rows, the table, the block counts
struct MapRowsLayout { size_t keys, sums, count, mask, last_stamp, born, bytes; };
MapRowsLayout map_rows_layout(int max_rows) {
    const size_t R = (size_t)max_rows;
    MapRowsLayout L; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 127) & ~(size_t)127; return o; };   // (arrays start on cache lines)
    L.sums = take(64 * R); L.keys = take(8 * R); L.mask = take(8 * R); L.count = take(4 * R); L.last_stamp = take(4 * R); L.born = take(4 * R); L.bytes = at;
    return L;
}
inline size_t map_table_keys(int max_rows) { return (16 * (size_t)max_rows + 127) & ~(size_t)127; }
inline size_t map_table_rows(int max_rows) { return (8 * (size_t)max_rows + 127) & ~(size_t)127; }
inline size_t map_blocks(cvo_maps m) { return (size_t)std::max(m->max_rows, m->r->max_points) / 256 + 1; }
void maps_release(cvo_maps m) {
    (void)hipSetDevice(m->r->device);
    (void)hipStreamSynchronize(m->r->stream);
    if (m->mem) (void)hipFree(m->mem);
    if (m->d_desc) (void)hipFree(m->d_desc);
    if (m->h_desc) (void)hipHostFree(m->h_desc);
    --m->r->live_maps;
    delete m;
}
MapRows map_rows_at(char* base, const MapRowsLayout& L) {
    MapRows R;
    R.keys = reinterpret_cast<unsigned long long*>(base + L.keys); R.sums = reinterpret_cast<long long*>(base + L.sums);
    R.count = reinterpret_cast<unsigned*>(base + L.count); R.mask = reinterpret_cast<unsigned long long*>(base + L.mask);
    R.last_stamp = reinterpret_cast<int*>(base + L.last_stamp); R.born = reinterpret_cast<int*>(base + L.born);
    return R;
}
// map k's share of the object's memory
char* map_base(cvo_maps m, int k) {
    char* base = m->mem + up16(4 * (size_t)m->max_maps) + (size_t)k * m->map_bytes;
    return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 127) & ~(uintptr_t)127);
}
// Where map k lies now -- the side that holds its rows and the other, the table behind both, `live`, the rows and the slots -- for every record
// that names a map; block_heads: the block counts behind the table, if asked for.  Compact and restore flip the side; nothing else reads it.
MapPlace map_place(cvo_maps m, int k, int** block_heads = nullptr) {
    const MapRowsLayout L = map_rows_layout(m->max_rows);
    char* base = map_base(m, k);
    char* table = base + 2 * L.bytes;
    MapPlace P;
    P.at = map_rows_at(base + (m->side[k] ? L.bytes : 0), L); P.to = map_rows_at(base + (m->side[k] ? 0 : L.bytes), L);
    P.tkeys = reinterpret_cast<unsigned long long*>(table); P.trow = reinterpret_cast<int*>(table + map_table_keys(m->max_rows));
    P.live = m->d_live + k;
    P.rows = m->rows[k]; P.slots = 2 * m->max_rows;
    if (block_heads) *block_heads = reinterpret_cast<int*>(table + map_table_keys(m->max_rows) + map_table_rows(m->max_rows));
    return P;
}
// record q of a call: map `k` as it stands, its figures at the reducer's counts 4 q ..; everything a single kind of call sets stays 0
MapDesc& maps_desc(cvo_maps m, int q, int k) {
    MapDesc& D = m->h_desc[q];
    std::memset(&D, 0, sizeof(D));
    static_cast<MapPlace&>(D) = map_place(m, k, &D.block_heads);
    D.total = m->r->d_total + MAP_FIGURES * q;
    return D;
}
// the range of a row filter's min_views (extract's, compact's keep rule, a view's and a probe's), `who`: "map 3: "
int maps_check_filter(const std::string& who, int min_views) {
    if (min_views < 0 || min_views > FUSE_MAX_MEMBERS) return fail(CVO_ERR_INVALID, who + "min_views " + std::to_string(min_views) + " is outside 0 .. 64");
    return CVO_OK;
}
inline MapRowFilter map_row_filter(const cvo_map_filter& f) { return MapRowFilter{f.min_points, f.min_views, f.min_last_stamp}; }
int maps_check_list(cvo_maps m, int count, const int* maps, const char* what) {
    if (!m) return fail(CVO_ERR_INVALID, "null maps object");
    if (count < 1 || count > m->max_maps) return fail(CVO_ERR_INVALID, std::string(what) + " " + std::to_string(count) + " is outside 1 .. max_maps " + std::to_string(m->max_maps));
    if (!maps) return fail(CVO_ERR_INVALID, "null argument: maps");
    std::vector<char> seen(m->max_maps, 0);
    for (int q = 0; q < count; ++q) {
        if (maps[q] < 0 || maps[q] >= m->max_maps) return fail(CVO_ERR_INVALID, "maps[" + std::to_string(q) + "] " + std::to_string(maps[q]) + " is outside 0 .. " + std::to_string(m->max_maps - 1));
        if (seen[maps[q]]) return fail(CVO_ERR_INVALID, "map " + std::to_string(maps[q]) + " appears twice in the call");
        seen[maps[q]] = 1;
    }
    return CVO_OK;
}
int maps_check_update(cvo_maps m, int groups, const int* maps, const int* group_first, const int* stamps, int sign) {
    int rc = maps_check_list(m, groups, maps, "groups"); if (rc) return rc;
    if (sign != CVO_MAP_INTEGRATE && sign != CVO_MAP_REMOVE && sign != CVO_MAP_REMOVE_PRESENT)
        return fail(CVO_ERR_INVALID, "sign " + std::to_string(sign) + " is neither +1 (integrate), -1 (remove) nor -2 (remove what is still there)");
    if (!group_first || !stamps) return fail(CVO_ERR_INVALID, "null argument");
    return CVO_OK;
}
int maps_check_stamps(int groups, const int* group_first, const int* stamps) {
    for (int g = 0; g < groups; ++g)
        for (int k = group_first[g]; k < group_first[g + 1]; ++k)
            if (stamps[k] < 0) return fail(CVO_ERR_INVALID, "group " + std::to_string(g) + " member " + std::to_string(k - group_first[g]) + ": stamp " + std::to_string(stamps[k]) + " is negative");
    return CVO_OK;
}
// the fuser's own validation of an update's members: a MEAN fusion at the maps' voxel that keeps every cell and writes nothing
int maps_check_clouds(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_member* members, const int* stamps, int sign) {
    int rc = maps_check_update(m, groups, maps, group_first, stamps, sign); if (rc) return rc;
    const cvo_fuse_params P = {m->voxel, CVO_REDUCE_MEAN, 1, 1};
    std::vector<cvo_fused_cloud> none(groups); std::memset(none.data(), 0, sizeof(cvo_fused_cloud) * groups);
    if ((rc = fuse_check(m->r, groups, group_first, members, &P, none.data()))) return rc;
    return maps_check_stamps(groups, group_first, stamps);
}
int maps_check_frames(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step,
                      const cvo_camera* cams, const int* stamps, int sign) {
    int rc = maps_check_update(m, groups, maps, group_first, stamps, sign); if (rc) return rc;
    const cvo_fuse_params P = {m->voxel, CVO_REDUCE_MEAN, 1, 1};
    std::vector<cvo_fused_cloud> none(groups); std::memset(none.data(), 0, sizeof(cvo_fused_cloud) * groups);
    if ((rc = fuse_frames_check(m->r, groups, group_first, members, width, height, step, cams, &P, none.data()))) return rc;
    return maps_check_stamps(groups, group_first, stamps);
}
// the edges of a call over MapDesc records: they are copied beside the reducer's table (fuse_bytes of it; 0: none), four figures per map
int maps_run(cvo_maps m, int n_maps, size_t fuse_bytes, void* stream, const std::function<hipError_t()>& queue) {
    CallEdges c{"resident maps"};
    c.table_bytes = fuse_bytes; c.own_host = m->h_desc; c.own_dev = m->d_desc; c.own_bytes = sizeof(MapDesc) * (size_t)n_maps;
    c.zero_figures = c.read_figures = MAP_FIGURES * n_maps;
    return run_call(m->r, c, stream, queue);
}
// src's item k is member k of the call, pose(k) its 12 floats.  A group with points gets a FuseGroupDesc, its members with points FuseMemberDescs
// behind them (fuse_points' tables), and its map a MapDesc; a group without points changes nothing.
int maps_update(cvo_maps m, int groups, const int* maps, const int* group_first, const PointSource& src, const std::function<const float*(int)>& pose,
                const int* stamps, int sign, void* stream) {
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    const MapLayout L = map_layout(r->max_points);
    std::vector<int> of; of.reserve(groups);
    int live_members = 0;
    for (int g = 0; g < groups; ++g) {
        const int before = live_members;
        for (int k = group_first[g]; k < group_first[g + 1]; ++k) live_members += src.n(k) > 0;
        if (live_members > before) of.push_back(g);
    }
    const int live = (int)of.size();
    if (live == 0) return CVO_OK;
    DescTable tab{r};
    FuseGroupDesc* hg; const FuseGroupDesc* dg; FuseMemberDesc* hm; const FuseMemberDesc* dm; FrameDesc* hf = nullptr; const FrameDesc* df = nullptr;
    int rc;
    if ((rc = tab.take(live, &hg, &dg)) || (rc = tab.take(live_members, &hm, &dm))) return rc;
    if (src.frames() && (rc = tab.take(live_members, &hf, &df))) return rc;
    int n_max = 0, group_max = 0, qm = 0;
    for (int q = 0; q < live; ++q) {
        const int g = of[q];
        FuseGroupDesc& G = hg[q];
        std::memset(&G, 0, sizeof(G));                                // (no output arrays: the cells stay in the scratch)
        MapDesc& D = maps_desc(m, q, maps[g]);
        G.first_member = qm;
        int at = 0, blocks = 0;
        for (int k = group_first[g]; k < group_first[g + 1]; ++k) {
            D.stamps[k - group_first[g]] = stamps[k];
            const int n = src.n(k);
            if (n == 0) continue;
            FuseMemberDesc& M = hm[qm];
            src.fill(k, M, hf, qm);
            ++qm;
            std::memcpy(M.pose, pose(k), sizeof(M.pose));
            M.group = q; M.base = at; M.first_block = blocks; M.n = n; M.bit = k - group_first[g]; M.pad_ = 0;
            at += n; blocks += (n + 255) / 256;
            n_max = std::max(n_max, n);
        }
        char* base = static_cast<char*>(r->scratch) + (size_t)q * L.bytes;
        G.keys = reinterpret_cast<unsigned long long*>(base + L.keys); G.masks = reinterpret_cast<unsigned long long*>(base + L.masks);
        G.lowest = reinterpret_cast<unsigned*>(base + L.lowest); G.members = reinterpret_cast<unsigned*>(base + L.members);
        G.row = reinterpret_cast<int*>(base + L.row); G.slot_of = reinterpret_cast<int*>(base + L.slot_of);
        G.block_heads = reinterpret_cast<int*>(base + L.block_heads); G.row_slot = reinterpret_cast<int*>(base + L.row_slot);
        G.sums = reinterpret_cast<long long*>(base + L.sums); G.best = reinterpret_cast<unsigned long long*>(base + L.best);
        G.total = D.total;
        G.n = at; G.slots = 2 * at; G.cap = at; G.rows_cap = at;
        G.n_blocks = blocks; G.n_members = qm - G.first_member;
        D.cell_row = reinterpret_cast<int*>(base + L.cell_row);
        D.group = q; D.sign = sign;
        group_max = std::max(group_max, at);
    }
    const float voxel = m->voxel;
    if ((rc = maps_run(m, live, tab.used, stream, [&] {
            const hipError_t e = launch_fuse_cells(dg, live, dm, df, live_members, n_max, 2 * group_max, group_max, voxel, r->stream);
            return e != hipSuccess ? e : launch_map_lookup(m->d_desc, live, dg, group_max, r->stream); })))
        return rc;
    // the figures: refuse with every map as it was, or go on
    int cells_max = 0;
    for (int q = 0; q < live; ++q) {
        const int* fig = r->h_total + MAP_FIGURES * q;
        const int k = maps[of[q]];
        const std::string who = "map " + std::to_string(k) + " (group " + std::to_string(of[q]) + "): ";
        if (fig[2] & 1) return fail(CVO_ERR_INVALID, who + "the integration would take a cell's count above " + std::to_string(CVO_MAP_MAX_COUNT));
        if (fig[2] & 2) return fail(CVO_ERR_INVALID, who + "the removal names a cell that is absent from the map");
        if (fig[2] & 4) return fail(CVO_ERR_INVALID, who + "the removal takes more members out of a cell than its count");
        if (fig[2] & 8) return fail(CVO_ERR_INVALID, who + "the removal's group is partly present in a row: some of the stamps of the members that touch a cell are in its view_mask, some are not");
        if ((long long)m->rows[k] + fig[1] > m->max_rows)
            return fail(CVO_ERR_INVALID, who + "its " + std::to_string(m->rows[k]) + " rows and the integration's " + std::to_string(fig[1]) + " new cells are above max_rows " + std::to_string(m->max_rows));
        cells_max = std::max(cells_max, fig[0]);
    }
    const hipError_t e = launch_map_merge(m->d_desc, live, dg, cells_max, false, r->stream);   // behind it runs every later call on the reducer
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("resident maps kernel launch: ") + hipGetErrorString(e));
    for (int q = 0; q < live; ++q) m->rows[maps[of[q]]] += r->h_total[MAP_FIGURES * q + 1];
    return CVO_OK;
}
int maps_check_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter, const cvo_map_cloud* dst) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    if (!filter || !dst) return fail(CVO_ERR_INVALID, "null argument");
    for (int q = 0; q < count; ++q) {
        const std::string who = "map " + std::to_string(maps[q]) + ": ";
        const cvo_map_cloud& d = dst[q];
        if ((rc = maps_check_filter(who, filter[q].min_views))) return rc;
        if (d.cap < 0 || d.cap > 65535) return fail(CVO_ERR_INVALID, who + "cap " + std::to_string(d.cap) + " is outside 0 .. 65535");
        if (d.cap > 0 && !d.xyz) return fail(CVO_ERR_INVALID, who + "dst xyz is null with cap " + std::to_string(d.cap));
        if (d.cap > 0 && !d.feat) return fail(CVO_ERR_INVALID, who + "dst feat is null with cap " + std::to_string(d.cap));
        if ((rc = check_out_arrays(m->r->device, who, {{d.xyz, 12ll * d.cap, 4, "dst xyz", false}, {d.feat, 20ll * d.cap, 4, "dst feat", false},
                {d.count, 4ll * d.cap, 4, "dst count", false}, {d.views, 4ll * d.cap, 4, "dst views", false}, {d.view_mask, 8ll * d.cap, 8, "dst view_mask", false},
                {d.last_stamp, 4ll * d.cap, 4, "dst last_stamp", false}, {d.born, 4ll * d.cap, 4, "dst born", false}, {d.row, 4ll * d.cap, 4, "dst row", false}})))
            return rc;
    }
    return CVO_OK;
}
int maps_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter, const cvo_map_cloud* dst, int* n_out, void* stream) {
    if (!n_out) return fail(CVO_ERR_INVALID, "null argument: n_out");
    HIP_TRY(hipSetDevice(m->r->device));
    int rows_max = 0, cap_max = 0;
    for (int q = 0; q < count; ++q) {
        n_out[q] = 0;
        MapDesc& D = maps_desc(m, q, maps[q]);
        const cvo_map_cloud& d = dst[q];
        D.out_xyz = static_cast<float*>(d.xyz); D.out_feat = static_cast<float*>(d.feat); D.out_count = static_cast<int*>(d.count);
        D.out_views = static_cast<int*>(d.views); D.out_view_mask = static_cast<unsigned long long*>(d.view_mask);
        D.out_last_stamp = static_cast<int*>(d.last_stamp); D.out_born = static_cast<int*>(d.born); D.out_row = static_cast<int*>(d.row);
        D.cap = d.cap; D.filter = map_row_filter(filter[q]);
        rows_max = std::max(rows_max, D.rows); cap_max = std::max(cap_max, d.cap);
    }
    if (rows_max == 0) return CVO_OK;
    int rc = maps_run(m, count, 0, stream, [&] { return launch_map_extract(m->d_desc, count, rows_max, cap_max > 0, m->r->stream); });
    if (rc) return rc;
    for (int q = 0; q < count; ++q) n_out[q] = m->r->h_total[MAP_FIGURES * q];
    return CVO_OK;
}
int maps_check_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep, const void* const* drop, void* const* new_row) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    if (!keep) return fail(CVO_ERR_INVALID, "null argument: keep");
    for (int q = 0; q < count; ++q) {
        const std::string who = "map " + std::to_string(maps[q]) + ": ";
        if ((rc = maps_check_filter(who, keep[q].min_views))) return rc;
        const long long rows = m->rows[maps[q]];
        if ((rc = check_out_arrays(m->r->device, who, {{drop ? drop[q] : nullptr, rows, 1, "drop", false}, {new_row ? new_row[q] : nullptr, 4 * rows, 4, "new_row", false}}))) return rc;
    }
    return CVO_OK;
}
int maps_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep, const void* const* drop, void* const* new_row, int* rows_out, void* stream) {
    HIP_TRY(hipSetDevice(m->r->device));
    int rows_max = 0;
    for (int q = 0; q < count; ++q) {
        if (rows_out) rows_out[q] = 0;
        MapDesc& D = maps_desc(m, q, maps[q]);
        D.drop = drop ? static_cast<const uint8_t*>(drop[q]) : nullptr; D.new_row = new_row ? static_cast<int*>(new_row[q]) : nullptr;
        D.filter.min_last_stamp = keep[q].min_last_stamp; D.filter.min_views = keep[q].min_views; D.probation_from = keep[q].probation_from;
        rows_max = std::max(rows_max, D.rows);
    }
    if (rows_max == 0) return CVO_OK;
    int rc = maps_run(m, count, 0, stream, [&] { return launch_map_compact(m->d_desc, count, rows_max, m->r->stream); });
    if (rc) return rc;
    for (int q = 0; q < count; ++q) {
        const int k = maps[q];
        if (m->rows[k] > 0) { m->rows[k] = m->r->h_total[MAP_FIGURES * q]; m->side[k] ^= 1; }   // (a map without rows was not touched)
        if (rows_out) rows_out[q] = m->rows[k];
    }
    return CVO_OK;
}
// -- viewing maps (cvo_view_kernels.hip with the map as the point source; cvo_hip.h, "Viewing maps").  A list of views, not of maps: a map may
// stand in several.  View q takes region q of the reducer's scratch, laid out from the call's own sizes -- the z-buffer of `cells` z-cells, and
// for R = the most rows among the call's maps a code word per row and the counts of its ceil(R / 256) blocks -- and five of the reducer's
// counts, as view_points does.  The maps are read only.
// A region here is an equal share of the whole scratch (384 bytes per point of max_points), not the 120 bytes per point of a reduction's region:
// a map may have many more rows than max_points.
inline size_t map_view_region(cvo_reducer r) { return (r->scratch_bytes / (size_t)r->max_clouds) & ~(size_t)15; }
struct MapViewLayout { size_t code, block_heads, block_relations, bytes; };   // (the z-buffer is at 0)
MapViewLayout map_view_layout(long long cells, int rows_max) {
    const size_t R = (size_t)rows_max, B = (R + 255) / 256;
    MapViewLayout L;
    L.code = up16(8 * (size_t)cells); L.block_heads = L.code + up16(4 * R); L.block_relations = L.block_heads + up16(4 * B); L.bytes = L.block_relations + up16(16 * B);
    return L;
}
int maps_check_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                    const cvo_viewed_cloud* dst, void* const* carve) {
    if (!m) return fail(CVO_ERR_INVALID, "null maps object");
    cvo_reducer r = m->r;
    if (views < 1 || views > r->max_clouds) return fail(CVO_ERR_INVALID, "views " + std::to_string(views) + " is outside 1 .. the reducer's max_clouds " + std::to_string(r->max_clouds));
    if (!v || !cams || !p || !dst) return fail(CVO_ERR_INVALID, "null argument");
    int rc = view_check_params(r, *p); if (rc) return rc;
    if (carve && !observed) return fail(CVO_ERR_INVALID, "carve is set but observed is null");
    const long long cells = (long long)frame_sub(p->width, p->cell) * frame_sub(p->height, p->cell);
    int rows_max = 0;
    for (int k = 0; k < views; ++k) {
        const std::string who = "view " + std::to_string(k) + ": ";
        if (v[k].map < 0 || v[k].map >= m->max_maps) return fail(CVO_ERR_INVALID, who + "map " + std::to_string(v[k].map) + " is outside 0 .. " + std::to_string(m->max_maps - 1));
        if ((rc = maps_check_filter(who, v[k].filter.min_views))) return rc;
        if ((rc = fuse_check_pose(v[k].pose, who)) || (rc = frames_check_camera(cams, v[k].cam, who))) return rc;
        const long long rows = m->rows[v[k].map];
        rows_max = std::max(rows_max, (int)rows);
        const cvo_viewed_cloud& d = dst[k];
        if (d.cap < 0 || d.cap > 65535) return fail(CVO_ERR_INVALID, who + "cap " + std::to_string(d.cap) + " is outside 0 .. 65535");
        if (d.cap > 0 && !d.xyz) return fail(CVO_ERR_INVALID, who + "dst xyz is null with cap " + std::to_string(d.cap));
        if (d.cap > 0 && !d.feat) return fail(CVO_ERR_INVALID, who + "dst feat is null with cap " + std::to_string(d.cap));
        if (d.relation && !observed) return fail(CVO_ERR_INVALID, who + "dst relation is set but observed is null");
        if (observed && (rc = view_check_observed(r->device, observed[k], p->width, p->height, who))) return rc;
        if ((rc = check_out_arrays(r->device, who, {{d.xyz, 12ll * d.cap, 4, "dst xyz", false}, {d.feat, 20ll * d.cap, 4, "dst feat", false},
                                                    {d.source, 4ll * d.cap, 4, "dst source", false}, {d.pixel, 4ll * d.cap, 4, "dst pixel", false},
                                                    {d.relation, 4ll * d.cap, 4, "dst relation", false}, {d.map, 4 * rows, 4, "dst map", false},
                                                    {d.depth, 4 * cells, 4, "dst depth", false}, {d.index, 4 * cells, 4, "dst index", false},
                                                    {carve ? carve[k] : nullptr, rows, 1, "carve", false}}))) return rc;
    }
    const size_t need = map_view_layout(cells, rows_max).bytes;
    if (need > map_view_region(r))
        return fail(CVO_ERR_INVALID, "a view of " + std::to_string(cells) + " z-cells over " + std::to_string(rows_max) + " rows takes " + std::to_string(need) +
                                     " bytes of scratch, above the " + std::to_string(map_view_region(r)) + " bytes of a region of the reducer: create the reducer with a larger max_points");
    if ((size_t)VIEW_COUNTS * views > (size_t)r->max_clouds * CVO_REDUCE_MAX_VOXELS) return fail(CVO_ERR_INVALID, "the reducer's counts have no room");   // (never: 5 of 16 per cloud)
    return CVO_OK;
}
// every view gets a record, an empty map too: its depth and index images are written all the same
int maps_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
              const cvo_viewed_cloud* dst, void* const* carve, int* n_out, int* relation_counts, void* stream) {
    if (!n_out) return fail(CVO_ERR_INVALID, "null argument: n_out");
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    DescTable tab{r};
    ViewDesc* h; const ViewDesc* d; MapViewSrc* hs; const MapViewSrc* ds;
    int rc;
    if ((rc = tab.take(views, &h, &d)) || (rc = tab.take(views, &hs, &ds))) return rc;
    ViewParams P;
    P.width = p->width; P.height = p->height; P.cell = p->cell; P.mode = p->mode; P.gw = frame_sub(p->width, p->cell); P.gh = frame_sub(p->height, p->cell);
    P.z_near = p->z_near; P.z_far = p->z_far; P.slack = p->slack; P.depth_tol = p->depth_tol;
    int n_max = 0; bool images = false;
    for (int q = 0; q < views; ++q) n_max = std::max(n_max, m->rows[v[q].map]);
    const MapViewLayout L = map_view_layout((long long)P.gw * P.gh, n_max);
    for (int q = 0; q < views; ++q) {
        ViewDesc& V = h[q]; MapViewSrc& S = hs[q];
        std::memset(&V, 0, sizeof(V));                                // (no cloud: the rows are the points)
        const int k = v[q].map;
        const cvo_camera& c = cams[v[q].cam];
        S.map = map_place(m, k);
        S.carve = carve ? static_cast<uint8_t*>(carve[q]) : nullptr;
        S.filter = map_row_filter(v[q].filter); S.pad_ = 0;
        std::memcpy(V.pose, v[q].pose, sizeof(V.pose));
        V.fx = c.fx; V.fy = c.fy; V.cx = c.cx; V.cy = c.cy; V.scaling_factor = c.scaling_factor; V.n = S.map.rows;
        char* base = static_cast<char*>(r->scratch) + (size_t)q * map_view_region(r);
        V.zbuf = reinterpret_cast<unsigned long long*>(base); V.code = reinterpret_cast<int*>(base + L.code); V.block_heads = reinterpret_cast<int*>(base + L.block_heads);
        V.block_relations = reinterpret_cast<int*>(base + L.block_relations);
        V.total = r->d_total + VIEW_COUNTS * q; V.relation_counts = V.total + 1;
        V.observed = observed ? static_cast<const uint8_t*>(observed[q].depth16) : nullptr;
        V.observed_pitch = observed && observed[q].depth_pitch ? observed[q].depth_pitch : 2ll * p->width;
        const cvo_viewed_cloud& o = dst[q];
        V.out_xyz = static_cast<float*>(o.xyz); V.out_feat = static_cast<float*>(o.feat); V.out_source = static_cast<int*>(o.source);
        V.out_pixel = static_cast<int*>(o.pixel); V.out_relation = static_cast<int*>(o.relation); V.out_map = static_cast<int*>(o.map);
        V.out_depth = static_cast<float*>(o.depth); V.out_index = static_cast<int*>(o.index);
        V.cap = o.cap;
        images = images || o.depth || o.index;
    }
    if ((rc = reducer_run(r, tab.used, VIEW_COUNTS * views, stream, [&] { return launch_view_maps(d, ds, views, n_max, P, observed != nullptr, images, r->stream); }))) return rc;
    for (int q = 0; q < views; ++q) {
        n_out[q] = r->h_total[VIEW_COUNTS * q];
        if (relation_counts)
            for (int k = 0; k < 4; ++k) relation_counts[4 * q + k] = observed ? r->h_total[VIEW_COUNTS * q + 1 + k] : 0;
    }
    return CVO_OK;
}
// -- probing maps (cvo_probe_kernels.hip; cvo_hip.h, "Probing maps").  A list of probes, not of maps: a map may stand in several.  Probe q takes
// region q of the reducer's scratch (map_view_region: an equal share) for the four counts of each of its member's 256-point blocks, and four of
// the reducer's counts.  A member is not bound by max_points: nothing of the scratch grows with it but those 16 bytes per block.  The maps are
// read only, where they lie: the table, and the rows of the side that holds them.
constexpr int PROBE_COUNTS = 4;
inline size_t probe_blocks_bytes(long long n) { return 16 * (size_t)((n + 255) / 256); }
int maps_check_probe_head(cvo_maps m, int probes, const cvo_map_probe* p, const void* members, const cvo_probed_points* dst) {
    if (!m) return fail(CVO_ERR_INVALID, "null maps object");
    if (probes < 1 || probes > m->r->max_clouds)
        return fail(CVO_ERR_INVALID, "probes " + std::to_string(probes) + " is outside 1 .. the reducer's max_clouds " + std::to_string(m->r->max_clouds));
    if (!p || !members || !dst) return fail(CVO_ERR_INVALID, "null argument");
    return CVO_OK;
}
// what both probing calls check behind their members; n_of(k): the points of probe k's member
int maps_check_probe_tail(cvo_maps m, int probes, const cvo_map_probe* p, const std::function<long long(int)>& n_of, const cvo_probed_points* dst) {
    cvo_reducer r = m->r;
    long long n_max = 0;
    int rc;
    for (int k = 0; k < probes; ++k) {
        const std::string who = "probe " + std::to_string(k) + ": ";
        if (p[k].map < 0 || p[k].map >= m->max_maps) return fail(CVO_ERR_INVALID, who + "map " + std::to_string(p[k].map) + " is outside 0 .. " + std::to_string(m->max_maps - 1));
        if (p[k].reach != 0 && p[k].reach != 1) return fail(CVO_ERR_INVALID, who + "reach " + std::to_string(p[k].reach) + " is neither 0 nor 1");
        if ((rc = maps_check_filter(who, p[k].filter.min_views))) return rc;
        const long long n = n_of(k), rows = m->rows[p[k].map];
        const cvo_probed_points& d = dst[k];
        const struct { const void* ptr; const char* name; } needs_row[4] = {{d.dist2, "dist2"}, {d.count, "count"}, {d.views, "views"}, {d.last_stamp, "last_stamp"}};
        for (const auto& x : needs_row)
            if (x.ptr && !d.row) return fail(CVO_ERR_INVALID, who + "dst " + x.name + " is set but dst row is null");
        if ((rc = check_out_arrays(r->device, who, {{d.row, 4 * n, 4, "dst row", false}, {d.dist2, 4 * n, 4, "dst dist2", false}, {d.count, 4 * n, 4, "dst count", false},
                                                    {d.views, 4 * n, 4, "dst views", false}, {d.last_stamp, 4 * n, 4, "dst last_stamp", false},
                                                    {d.hit, rows, 1, "dst hit", false}}))) return rc;
        n_max = std::max(n_max, n);
    }
    if (probe_blocks_bytes(n_max) > map_view_region(r))
        return fail(CVO_ERR_INVALID, "a probe of " + std::to_string(n_max) + " points takes " + std::to_string(probe_blocks_bytes(n_max)) + " bytes of scratch, above the " +
                                     std::to_string(map_view_region(r)) + " bytes of a region of the reducer: create the reducer with a larger max_points");
    if ((size_t)PROBE_COUNTS * probes > (size_t)r->max_clouds * CVO_REDUCE_MAX_VOXELS) return fail(CVO_ERR_INVALID, "the reducer's counts have no room");   // (never: 4 of 16 per cloud)
    return CVO_OK;
}
int maps_check_probe_clouds(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_member* members, const cvo_probed_points* dst) {
    int rc = maps_check_probe_head(m, probes, p, members, dst); if (rc) return rc;
    std::vector<cvo_device_cloud> clouds(probes); std::vector<std::string> names(probes);
    for (int k = 0; k < probes; ++k) {
        clouds[k] = members[k].cloud;
        names[k] = "probe " + std::to_string(k) + ": ";
        if ((rc = fuse_check_pose(members[k].pose, names[k]))) return rc;
    }
    if ((rc = check_device_clouds(m->r->device, probes, clouds.data(), CVO_REDUCE_MAX_POINTS, names.data()))) return rc;
    return maps_check_probe_tail(m, probes, p, [&](int k) { return (long long)members[k].cloud.n; }, dst);
}
int maps_check_probe_frames(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                            const cvo_probed_points* dst) {
    int rc = maps_check_probe_head(m, probes, p, members, dst); if (rc) return rc;
    std::vector<cvo_device_image> images(probes);
    for (int k = 0; k < probes; ++k) images[k] = members[k].image;
    if ((rc = check_device_images(m->r->device, probes, images.data(), width, height))) return rc;   // ("image k": the probe's place in the call)
    if (step < 1 || step > 16) return fail(CVO_ERR_INVALID, "step " + std::to_string(step) + " is outside 1 .. 16");
    const long long n = (long long)frame_sub(width, step) * frame_sub(height, step);
    if (n > CVO_REDUCE_MAX_POINTS) return fail(CVO_ERR_INVALID, "a frame's " + std::to_string(n) + " points at step " + std::to_string(step) + " are above " + std::to_string(CVO_REDUCE_MAX_POINTS));
    if (!cams) return fail(CVO_ERR_INVALID, "null argument: cams");
    for (int k = 0; k < probes; ++k) {
        const std::string who = "probe " + std::to_string(k) + ": ";
        if ((rc = fuse_check_pose(members[k].pose, who)) || (rc = frames_check_camera(cams, members[k].cam, who))) return rc;
    }
    return maps_check_probe_tail(m, probes, p, [&](int) { return n; }, dst);
}
// every probe gets a record, an empty member too: its four counts are 0 and its hit bytes are cleared all the same.  src's item k is probe k's
// member, pose(k) its 12 floats.  counts == nullptr and a stream: no host wait (run_call).
int maps_probe(cvo_maps m, int probes, const cvo_map_probe* p, const PointSource& src, const std::function<const float*(int)>& pose, const cvo_probed_points* dst,
               int* counts, void* stream) {
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    DescTable tab{r};
    ProbeDesc* h; const ProbeDesc* d; FrameDesc* hf = nullptr; const FrameDesc* df = nullptr;
    int rc;
    if ((rc = tab.take(probes, &h, &d))) return rc;
    if (src.frames() && (rc = tab.take(probes, &hf, &df))) return rc;
    int n_max = 0;
    for (int q = 0; q < probes; ++q) {
        ProbeDesc& D = h[q];
        std::memset(&D, 0, sizeof(D));
        src.fill(q, D, hf, q);
        std::memcpy(D.pose, pose(q), sizeof(D.pose));
        D.n = src.n(q); D.reach = p[q].reach;
        D.map = map_place(m, p[q].map);
        D.filter = map_row_filter(p[q].filter);
        const cvo_probed_points& o = dst[q];
        D.out_row = static_cast<int*>(o.row); D.out_dist2 = static_cast<float*>(o.dist2); D.out_count = static_cast<int*>(o.count);
        D.out_views = static_cast<int*>(o.views); D.out_last_stamp = static_cast<int*>(o.last_stamp);
        D.out_hit = D.map.rows > 0 ? static_cast<uint8_t*>(o.hit) : nullptr;
        D.block_counts = reinterpret_cast<int*>(static_cast<char*>(r->scratch) + (size_t)q * map_view_region(r));
        D.totals = r->d_total + PROBE_COUNTS * q;
        n_max = std::max(n_max, D.n);
    }
    CallEdges c{"map probe"};
    c.table_bytes = tab.used; c.read_figures = counts ? PROBE_COUNTS * probes : 0; c.may_return_early = true;
    if ((rc = run_call(r, c, stream, [&] {
            for (int q = 0; q < probes; ++q)                          // (the hit bytes cleared on the stream, in front of the kernels)
                if (h[q].out_hit) { const hipError_t e = hipMemsetAsync(h[q].out_hit, 0, (size_t)h[q].map.rows, r->stream); if (e != hipSuccess) return e; }
            return src.frames() ? launch_probe_frames(d, df, probes, n_max, m->voxel, r->stream) : launch_probe_clouds(d, probes, n_max, m->voxel, r->stream); })))
        return rc;
    if (counts) std::memcpy(counts, r->h_total, sizeof(int) * PROBE_COUNTS * (size_t)probes);
    return CVO_OK;
}
// -- saving and restoring maps (cvo_map_snapshot_kernels.hip; cvo_hip.h, "Saving and restoring maps").  The records are MapSnapDescs in the
// reducer's descriptor table (max_maps <= max_clouds of them: reducer_alloc's first term covers them), a restore's figures four ints per map of
// the call in the reducer's counts, as an update's.
static_assert(sizeof(MapSnapDesc) <= sizeof(ReduceDesc) + sizeof(FrameDesc), "a MapSnapDesc per map fits the reducer's descriptor table");
// max_clouds probes with a FrameDesc each, and max_clouds views with a MapViewSrc each: reducer_alloc's second term (16 CountDescs per cloud)
static_assert(sizeof(ProbeDesc) + sizeof(FrameDesc) <= CVO_REDUCE_MAX_VOXELS * sizeof(CountDesc), "a ProbeDesc and a FrameDesc per probe fit the reducer's descriptor table");
static_assert(sizeof(ViewDesc) + sizeof(MapViewSrc) <= CVO_REDUCE_MAX_VOXELS * sizeof(CountDesc), "a ViewDesc and a MapViewSrc per view fit the reducer's descriptor table");
int maps_check_snap_arrays(cvo_maps m, const std::string& who, const char* side, const cvo_map_snapshot& x, long long rows) {
    const bool need = rows > 0;
    const std::string s(side);
    const std::string names[6] = {s + " keys", s + " sums", s + " count", s + " view_mask", s + " last_stamp", s + " born"};
    return check_out_arrays(m->r->device, who, {{x.keys, 8 * rows, 8, names[0].c_str(), need}, {x.sums, 64 * rows, 8, names[1].c_str(), need},
                                                {x.count, 4 * rows, 4, names[2].c_str(), need}, {x.view_mask, 8 * rows, 8, names[3].c_str(), need},
                                                {x.last_stamp, 4 * rows, 4, names[4].c_str(), need}, {x.born, 4 * rows, 4, names[5].c_str(), need}});
}
int maps_check_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    if (!dst) return fail(CVO_ERR_INVALID, "null argument: dst");
    for (int q = 0; q < count; ++q) {
        const std::string who = "map " + std::to_string(maps[q]) + ": ";
        const int rows = m->rows[maps[q]];
        if (dst[q].rows < rows)
            return fail(CVO_ERR_INVALID, who + "dst rows " + std::to_string(dst[q].rows) + " (the arrays' capacity) is below the map's " + std::to_string(rows) + " rows: there are no partial snapshots");
        if ((rc = maps_check_snap_arrays(m, who, "dst", dst[q], rows))) return rc;
    }
    return CVO_OK;
}
int maps_check_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src, float voxel) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    if (!src) return fail(CVO_ERR_INVALID, "null argument: src");
    if (std::memcmp(&voxel, &m->voxel, sizeof(float)) != 0)
        return fail(CVO_ERR_INVALID, "voxel " + std::to_string(voxel) + " has not the bits of the object's voxel " + std::to_string(m->voxel) + ": a key means nothing at another cell size");
    for (int q = 0; q < count; ++q) {
        const std::string who = "map " + std::to_string(maps[q]) + ": ";
        if (src[q].rows < 0 || src[q].rows > m->max_rows)
            return fail(CVO_ERR_INVALID, who + "src rows " + std::to_string(src[q].rows) + " is outside 0 .. max_rows " + std::to_string(m->max_rows));
        if ((rc = maps_check_snap_arrays(m, who, "src", src[q], src[q].rows))) return rc;
    }
    return CVO_OK;
}
// record q of a call: map k as it stands and the caller's arrays x
void maps_snap_desc(cvo_maps m, MapSnapDesc& D, int q, int k, const cvo_map_snapshot& x) {
    std::memset(&D, 0, sizeof(D));
    static_cast<MapPlace&>(D) = map_place(m, k);
    D.ext.keys = static_cast<unsigned long long*>(x.keys); D.ext.sums = static_cast<long long*>(x.sums); D.ext.count = static_cast<unsigned*>(x.count);
    D.ext.mask = static_cast<unsigned long long*>(x.view_mask); D.ext.last_stamp = static_cast<int*>(x.last_stamp); D.ext.born = static_cast<int*>(x.born);
    D.figures = m->r->d_total + MAP_FIGURES * q;
}
// with a stream: no host wait (run_call)
int maps_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst, int* rows_out, void* stream) {
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    int rows_max = 0;
    for (int q = 0; q < count; ++q) {
        if (rows_out) rows_out[q] = m->rows[maps[q]];
        rows_max = std::max(rows_max, m->rows[maps[q]]);
    }
    if (rows_max == 0) return CVO_OK;
    DescTable tab{r};
    MapSnapDesc* h; const MapSnapDesc* d;
    int rc;
    if ((rc = tab.take(count, &h, &d))) return rc;
    for (int q = 0; q < count; ++q) maps_snap_desc(m, h[q], q, maps[q], dst[q]);
    CallEdges c{"map snapshot"};
    c.table_bytes = tab.used; c.may_return_early = true;
    return run_call(r, c, stream, [&] { return launch_map_snapshot(d, count, rows_max, r->stream); });
}
// Two steps, as an update: the rows written and tested on the side the map is not on, the table emptied and filled from them with the duplicate
// test; the call's one host wait, for the refusal bits; then the host flips the side -- or, on a refusal, queues the launches that make every
// listed map's table again from the rows it still has.  The caller's arrays are read in the first step only.
int maps_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src, void* stream) {
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    DescTable tab{r};
    MapSnapDesc* h; const MapSnapDesc* d;
    int rc;
    if ((rc = tab.take(count, &h, &d))) return rc;
    int new_max = 0, old_max = 0;
    for (int q = 0; q < count; ++q) {
        maps_snap_desc(m, h[q], q, maps[q], src[q]);
        h[q].ext_rows = src[q].rows;
        new_max = std::max(new_max, src[q].rows); old_max = std::max(old_max, h[q].rows);
    }
    CallEdges c{"map restore"};
    c.table_bytes = tab.used; c.zero_figures = c.read_figures = MAP_FIGURES * count;
    if ((rc = run_call(r, c, stream, [&] { return launch_map_restore(d, count, new_max, r->stream); }))) return rc;
    for (int q = 0; q < count; ++q) {
        const int bits = r->h_total[MAP_FIGURES * q + 1];
        if (!bits) continue;
        const hipError_t e = launch_map_restore_undo(d, count, old_max, 2 * m->max_rows, r->stream);   // behind it runs every later call on the reducer
        if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("map restore kernel launch: ") + hipGetErrorString(e));
        std::string what;
        const char* names[5] = {"a bad key", "a count above 16777215", "a negative stamp", "a sum out of bound", "a duplicate key"};
        for (int b = 0; b < 5; ++b)
            if (bits & (1 << b)) what += std::string(what.empty() ? "" : ", ") + names[b];
        return fail(CVO_ERR_INVALID, "map " + std::to_string(maps[q]) + " (entry " + std::to_string(q) + "): the rows are refused, bits " + std::to_string(bits) + ": " + what +
                                     "; every listed map is unchanged");
    }
    for (int q = 0; q < count; ++q) { m->rows[maps[q]] = src[q].rows; m->side[maps[q]] ^= 1; }
    return CVO_OK;
}
// -- merging maps (cvo_map_merge_kernels.hip; cvo_hip.h, "Merging maps").  An update whose call-cells come from a map's rows: merge q takes region q
// of the destination's reducer's scratch (map_layout: one row per point of max_points, so a source has at most max_points rows), a FuseGroupDesc
// and a MapMergeDesc in that reducer's descriptor table, the destination's MapDesc q and its four figures -- and from the lookup on it IS an update.
static_assert(sizeof(FuseGroupDesc) + sizeof(MapMergeDesc) <= CVO_REDUCE_MAX_VOXELS * sizeof(CountDesc), "a FuseGroupDesc and a MapMergeDesc per merge fit the reducer's descriptor table");
int maps_check_merge(cvo_maps dst, int count, const cvo_map_merge* merges, cvo_maps src, int level) {
    if (!dst || !src) return fail(CVO_ERR_INVALID, "null maps object");
    if (count < 1 || count > dst->max_maps) return fail(CVO_ERR_INVALID, "count " + std::to_string(count) + " is outside 1 .. the destination's max_maps " + std::to_string(dst->max_maps));
    if (!merges) return fail(CVO_ERR_INVALID, "null argument: merges");
    if (level < 0 || level > CVO_MAP_MERGE_MAX_LEVEL) return fail(CVO_ERR_INVALID, "level " + std::to_string(level) + " is outside 0 .. " + std::to_string(CVO_MAP_MERGE_MAX_LEVEL));
    if (dst->r->device != src->r->device)
        return fail(CVO_ERR_INVALID, "the source's device " + std::to_string(src->r->device) + " is not the destination's device " + std::to_string(dst->r->device));
    const float want = std::ldexp(src->voxel, level);
    if (std::memcmp(&want, &dst->voxel, sizeof(float)) != 0)
        return fail(CVO_ERR_INVALID, "the destination's voxel " + std::to_string(dst->voxel) + " has not the bits of the source's voxel " + std::to_string(src->voxel) + " times 2^" +
                                     std::to_string(level) + " (" + std::to_string(want) + "): cells nest only at exact powers of two");
    std::vector<char> is_dst(dst->max_maps, 0);
    for (int q = 0; q < count; ++q) {
        const cvo_map_merge& g = merges[q];
        const std::string who = "merge " + std::to_string(q) + ": ";
        if (g.dst_map < 0 || g.dst_map >= dst->max_maps) return fail(CVO_ERR_INVALID, who + "dst_map " + std::to_string(g.dst_map) + " is outside 0 .. " + std::to_string(dst->max_maps - 1));
        if (g.src_map < 0 || g.src_map >= src->max_maps) return fail(CVO_ERR_INVALID, who + "src_map " + std::to_string(g.src_map) + " is outside 0 .. " + std::to_string(src->max_maps - 1));
        if (is_dst[g.dst_map]) return fail(CVO_ERR_INVALID, who + "destination map " + std::to_string(g.dst_map) + " appears twice in the call");
        is_dst[g.dst_map] = 1;
        if (g.all_rows != 0 && g.all_rows != 1) return fail(CVO_ERR_INVALID, who + "all_rows " + std::to_string(g.all_rows) + " is neither 0 nor 1");
        int rc = maps_check_filter(who, g.filter.min_views); if (rc) return rc;
        if (src->rows[g.src_map] > dst->r->max_points)
            return fail(CVO_ERR_INVALID, who + "source map " + std::to_string(g.src_map) + " has " + std::to_string(src->rows[g.src_map]) + " rows, above the " + std::to_string(dst->r->max_points) +
                                         " (max_points) that a group's region of the destination's reducer forms cells for: compact the source, or create that reducer with a larger max_points");
    }
    if (src == dst)
        for (int q = 0; q < count; ++q)
            if (is_dst[merges[q].src_map])
                return fail(CVO_ERR_INVALID, "merge " + std::to_string(q) + ": map " + std::to_string(merges[q].src_map) + " is both a source and a destination of the call");
    return CVO_OK;
}
// Three steps, as an update: the call-cells formed from the sources' rows and looked up in the destinations; the call's one host wait, for the
// figures; then the launches that write the destinations.  The sources are read in the first step only.  A merge whose source has no rows changes nothing.
int maps_merge(cvo_maps dst, int count, const cvo_map_merge* merges, cvo_maps src, int level, void* stream) {
    cvo_reducer r = dst->r;
    HIP_TRY(hipSetDevice(r->device));
    const MapLayout L = map_layout(r->max_points);
    std::vector<int> of; of.reserve(count);
    for (int q = 0; q < count; ++q) if (src->rows[merges[q].src_map] > 0) of.push_back(q);
    const int live = (int)of.size();
    if (live == 0) return CVO_OK;
    DescTable tab{r};
    FuseGroupDesc* hg; const FuseGroupDesc* dg; MapMergeDesc* hs; const MapMergeDesc* ds;
    int rc;
    if ((rc = tab.take(live, &hg, &dg)) || (rc = tab.take(live, &hs, &ds))) return rc;
    int rows_max = 0;
    for (int q = 0; q < live; ++q) {
        const cvo_map_merge& g = merges[of[q]];
        FuseGroupDesc& G = hg[q];
        std::memset(&G, 0, sizeof(G));                                // (no output arrays, no members: the cells stay in the scratch)
        MapDesc& D = maps_desc(dst, q, g.dst_map);
        MapMergeDesc& S = hs[q];
        std::memset(&S, 0, sizeof(S));
        static_cast<MapPlace&>(S) = map_place(src, g.src_map);
        S.filter = map_row_filter(g.filter); S.all_rows = g.all_rows; S.level = level; S.group = q; S.figures = D.total;
        const int n = S.rows;
        char* base = static_cast<char*>(r->scratch) + (size_t)q * L.bytes;
        G.keys = reinterpret_cast<unsigned long long*>(base + L.keys); G.masks = reinterpret_cast<unsigned long long*>(base + L.masks);
        G.lowest = reinterpret_cast<unsigned*>(base + L.lowest); G.members = reinterpret_cast<unsigned*>(base + L.members);
        G.row = reinterpret_cast<int*>(base + L.row); G.slot_of = reinterpret_cast<int*>(base + L.slot_of);
        G.block_heads = reinterpret_cast<int*>(base + L.block_heads); G.row_slot = reinterpret_cast<int*>(base + L.row_slot);
        G.sums = reinterpret_cast<long long*>(base + L.sums); G.best = reinterpret_cast<unsigned long long*>(base + L.best);
        G.total = D.total;
        G.n = n; G.slots = 2 * n; G.cap = n; G.rows_cap = n;          // (n <= max_points: checked)
        G.n_blocks = (n + 255) / 256;
        D.cell_row = reinterpret_cast<int*>(base + L.cell_row);
        D.group = q; D.sign = CVO_MAP_INTEGRATE;
        rows_max = std::max(rows_max, n);
    }
    if ((rc = maps_run(dst, live, tab.used, stream, [&] {
            const hipError_t e = launch_map_merge_cells(ds, live, dg, rows_max, r->stream);
            return e != hipSuccess ? e : launch_map_lookup(dst->d_desc, live, dg, rows_max, r->stream); })))
        return rc;
    int cells_max = 0;
    for (int q = 0; q < live; ++q) {
        const int* fig = r->h_total + MAP_FIGURES * q;
        const int k = merges[of[q]].dst_map;
        const std::string who = "map " + std::to_string(k) + " (merge " + std::to_string(of[q]) + "): ";
        if (fig[2] & 1) return fail(CVO_ERR_INVALID, who + "the merge would take a cell's count above " + std::to_string(CVO_MAP_MAX_COUNT) + "; every map is unchanged");
        if ((long long)dst->rows[k] + fig[1] > dst->max_rows)
            return fail(CVO_ERR_INVALID, who + "its " + std::to_string(dst->rows[k]) + " rows and the merge's " + std::to_string(fig[1]) + " new cells are above max_rows " +
                                         std::to_string(dst->max_rows) + "; every map is unchanged");
        cells_max = std::max(cells_max, fig[0]);
    }
    const hipError_t e = launch_map_merge(dst->d_desc, live, dg, cells_max, true, r->stream);   // behind it runs every later call on the reducer
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("resident maps kernel launch: ") + hipGetErrorString(e));
    for (int q = 0; q < live; ++q) dst->rows[merges[of[q]].dst_map] += r->h_total[MAP_FIGURES * q + 1];
    return CVO_OK;
}
}  // namespace
}  // extern "C++"
int cvo_maps_create(cvo_reducer r, int max_maps, int max_rows, float voxel, cvo_maps* out) {
    if (!out) return fail(CVO_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!r) return fail(CVO_ERR_INVALID, "null reducer");
    if (max_maps < 1 || max_maps > r->max_clouds) return fail(CVO_ERR_INVALID, "max_maps " + std::to_string(max_maps) + " is outside 1 .. the reducer's max_clouds " + std::to_string(r->max_clouds));
    if (max_rows < 1 || max_rows > CVO_MAP_MAX_ROWS) return fail(CVO_ERR_INVALID, "max_rows " + std::to_string(max_rows) + " is outside 1 .. " + std::to_string(CVO_MAP_MAX_ROWS));
    if (!(std::isfinite(voxel) && voxel > 0.f)) return fail(CVO_ERR_INVALID, "voxel " + std::to_string(voxel) + " is not a finite size above 0");
    if ((size_t)max_maps * map_layout(r->max_points).bytes > r->scratch_bytes)
        return fail(CVO_ERR_INVALID, "the reducer's scratch (" + std::to_string(r->scratch_bytes) + " bytes) has no room for " + std::to_string(max_maps) + " groups of max_points " +
                                     std::to_string(r->max_points) + " (" + std::to_string(map_layout(r->max_points).bytes) + " bytes each): create the reducer with a larger max_points or more max_clouds");
    if ((size_t)max_maps * MAP_FIGURES > (size_t)r->max_clouds * CVO_REDUCE_MAX_VOXELS) return fail(CVO_ERR_INVALID, "the reducer's counts have no room");   // (never: 4 of 16 per cloud)
    HIP_TRY(hipSetDevice(r->device));
    cvo_maps m = new cvo_maps_s();
    m->r = r; m->max_maps = max_maps; m->max_rows = max_rows; m->voxel = voxel;
    m->rows.assign(max_maps, 0); m->side.assign(max_maps, 0);
    ++r->live_maps;
    m->map_bytes = 2 * map_rows_layout(max_rows).bytes + map_table_keys(max_rows) + map_table_rows(max_rows) + ((4 * map_blocks(m) + 127) & ~(size_t)127);
    m->bytes = up16(4 * (size_t)max_maps) + 128 + (size_t)max_maps * m->map_bytes;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->mem), m->bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->d_desc), sizeof(MapDesc) * (size_t)max_maps);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&m->h_desc), sizeof(MapDesc) * (size_t)max_maps, hipHostMallocDefault);
    if (e == hipSuccess) {                                            // every table empty (all ones), every live count 0
        m->d_live = reinterpret_cast<int*>(m->mem);
        e = hipMemsetAsync(m->mem, 0, up16(4 * (size_t)max_maps), r->stream);
        for (int k = 0; k < max_maps && e == hipSuccess; ++k) e = hipMemsetAsync(map_place(m, k).tkeys, 0xFF, 16 * (size_t)max_rows, r->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    }
    if (e != hipSuccess) { maps_release(m); return fail(CVO_ERR_HIP, std::string("cvo_maps_create: ") + hipGetErrorString(e)); }
    *out = m;
    return CVO_OK;
}
int cvo_maps_destroy(cvo_maps m) {
    if (m) maps_release(m);
    return CVO_OK;
}
int cvo_maps_info(cvo_maps m, int* max_maps, int* max_rows, float* voxel, long long* device_bytes) {
    if (!m) return fail(CVO_ERR_INVALID, "null maps object");
    if (max_maps) *max_maps = m->max_maps;
    if (max_rows) *max_rows = m->max_rows;
    if (voxel) *voxel = m->voxel;
    if (device_bytes) *device_bytes = (long long)(m->bytes + sizeof(MapDesc) * (size_t)m->max_maps);
    return CVO_OK;
}
int cvo_maps_clear(cvo_maps m, int count, const int* maps, void* stream) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    HIP_TRY(hipSetDevice(m->r->device));
    for (int q = 0; q < count; ++q) maps_desc(m, q, maps[q]);
    if ((rc = maps_run(m, count, 0, stream, [&] { return launch_map_clear(m->d_desc, sizeof(MapDesc), count, 2 * m->max_rows, m->r->stream); }))) return rc;
    for (int q = 0; q < count; ++q) m->rows[maps[q]] = 0;
    return CVO_OK;
}
int cvo_maps_rows(cvo_maps m, int count, const int* maps, int* rows, int* live_rows) {
    int rc = maps_check_list(m, count, maps, "count"); if (rc) return rc;
    for (int q = 0; q < count && rows; ++q) rows[q] = m->rows[maps[q]];
    if (!live_rows) return CVO_OK;
    cvo_reducer r = m->r;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpyAsync(r->h_total, m->d_live, sizeof(int) * (size_t)m->max_maps, hipMemcpyDeviceToHost, r->stream));   // (max_maps <= max_clouds ints)
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (int q = 0; q < count; ++q) live_rows[q] = r->h_total[maps[q]];
    return CVO_OK;
}
int cvo_check_maps_integrate_clouds(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_member* members, const int* stamps, int sign) {
    return maps_check_clouds(m, groups, maps, group_first, members, stamps, sign);
}
int cvo_check_maps_integrate_frames(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step,
                                    const cvo_camera* cams, const int* stamps, int sign) {
    return maps_check_frames(m, groups, maps, group_first, members, width, height, step, cams, stamps, sign);
}
int cvo_maps_integrate_clouds(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_member* members, const int* stamps, int sign,
                              void* cloud_stream) {
    int rc = maps_check_clouds(m, groups, maps, group_first, members, stamps, sign); if (rc) return rc;
    PointSource src; src.cloud = [&](int k) { return &members[k].cloud; };
    return maps_update(m, groups, maps, group_first, src, [&](int k) { return members[k].pose; }, stamps, sign, cloud_stream);
}
int cvo_maps_integrate_frames(cvo_maps m, int groups, const int* maps, const int* group_first, const cvo_fuse_frame* members, int width, int height, int step,
                              const cvo_camera* cams, const int* stamps, int sign, void* image_stream) {
    int rc = maps_check_frames(m, groups, maps, group_first, members, width, height, step, cams, stamps, sign); if (rc) return rc;
    PointSource src;
    src.frame = [&](int k, FrameDesc& F) { frame_desc(members[k].image, width, height, step, cams[members[k].cam], F); };
    src.frame_n = frame_sub(width, step) * frame_sub(height, step);
    return maps_update(m, groups, maps, group_first, src, [&](int k) { return members[k].pose; }, stamps, sign, image_stream);
}
int cvo_check_maps_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter, const cvo_map_cloud* dst) {
    return maps_check_extract(m, count, maps, filter, dst);
}
int cvo_maps_extract(cvo_maps m, int count, const int* maps, const cvo_map_filter* filter, const cvo_map_cloud* dst, int* n_out, void* stream) {
    int rc = maps_check_extract(m, count, maps, filter, dst); if (rc) return rc;
    return maps_extract(m, count, maps, filter, dst, n_out, stream);
}
int cvo_check_maps_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep, const void* const* drop, void* const* new_row) {
    return maps_check_compact(m, count, maps, keep, drop, new_row);
}
int cvo_maps_compact(cvo_maps m, int count, const int* maps, const cvo_map_keep* keep, const void* const* drop, void* const* new_row, int* rows_out, void* stream) {
    int rc = maps_check_compact(m, count, maps, keep, drop, new_row); if (rc) return rc;
    return maps_compact(m, count, maps, keep, drop, new_row, rows_out, stream);
}
int cvo_check_maps_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                        const cvo_viewed_cloud* dst, void* const* carve) {
    return maps_check_view(m, views, v, cams, p, observed, dst, carve);
}
int cvo_maps_view(cvo_maps m, int views, const cvo_map_view* v, const cvo_camera* cams, const cvo_view_params* p, const cvo_device_image* observed,
                  const cvo_viewed_cloud* dst, void* const* carve, int* n_out, int* relation_counts, void* stream) {
    int rc = maps_check_view(m, views, v, cams, p, observed, dst, carve); if (rc) return rc;
    return maps_view(m, views, v, cams, p, observed, dst, carve, n_out, relation_counts, stream);
}
int cvo_check_maps_probe_clouds(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_member* members, const cvo_probed_points* dst) {
    return maps_check_probe_clouds(m, probes, p, members, dst);
}
int cvo_check_maps_probe_frames(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                                const cvo_probed_points* dst) {
    return maps_check_probe_frames(m, probes, p, members, width, height, step, cams, dst);
}
int cvo_maps_probe_clouds(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_member* members, const cvo_probed_points* dst, int* counts, void* cloud_stream) {
    int rc = maps_check_probe_clouds(m, probes, p, members, dst); if (rc) return rc;
    PointSource src; src.cloud = [&](int k) { return &members[k].cloud; };
    return maps_probe(m, probes, p, src, [&](int k) { return members[k].pose; }, dst, counts, cloud_stream);
}
int cvo_maps_probe_frames(cvo_maps m, int probes, const cvo_map_probe* p, const cvo_fuse_frame* members, int width, int height, int step, const cvo_camera* cams,
                          const cvo_probed_points* dst, int* counts, void* image_stream) {
    int rc = maps_check_probe_frames(m, probes, p, members, width, height, step, cams, dst); if (rc) return rc;
    PointSource src;
    src.frame = [&](int k, FrameDesc& F) { frame_desc(members[k].image, width, height, step, cams[members[k].cam], F); };
    src.frame_n = frame_sub(width, step) * frame_sub(height, step);
    return maps_probe(m, probes, p, src, [&](int k) { return members[k].pose; }, dst, counts, image_stream);
}
int cvo_check_maps_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst) { return maps_check_snapshot(m, count, maps, dst); }
int cvo_maps_snapshot(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* dst, int* rows_out, void* stream) {
    int rc = maps_check_snapshot(m, count, maps, dst); if (rc) return rc;
    return maps_snapshot(m, count, maps, dst, rows_out, stream);
}
int cvo_check_maps_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src, float voxel) { return maps_check_restore(m, count, maps, src, voxel); }
int cvo_maps_restore(cvo_maps m, int count, const int* maps, const cvo_map_snapshot* src, float voxel, void* stream) {
    int rc = maps_check_restore(m, count, maps, src, voxel); if (rc) return rc;
    return maps_restore(m, count, maps, src, stream);
}
int cvo_check_maps_merge(cvo_maps dst, int count, const cvo_map_merge* merges, cvo_maps src, int level) { return maps_check_merge(dst, count, merges, src, level); }
int cvo_maps_merge(cvo_maps dst, int count, const cvo_map_merge* merges, cvo_maps src, int level, void* stream) {
    int rc = maps_check_merge(dst, count, merges, src, level); if (rc) return rc;
    return maps_merge(dst, count, merges, src, level, stream);
}
int cvo_batch_advance_staged(cvo_batch b, int* points_out) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    FrameStage& F = b->stage;
    if (!F.pending) return fail(CVO_ERR_INVALID, "nothing staged (cvo_batch_stage_images)");
    Lap lap(StepLaps::CONSUME);
    int rc = batch_settle(b); if (rc) return rc;
    if ((rc = stage_take(b))) return rc;                             // (fails before any slot changes)
    // the cloud objects the slots give up go to the pool and are written by a later stage: no launch may still read them then
    if (b->eng.launched && b->eng.last_stream) HIP_TRY(hipStreamSynchronize(b->eng.last_stream));
    auto give_up = [&](std::shared_ptr<Cloud>& c) { if (c && c.use_count() == 1) b->pool.push_back(c); c.reset(); };   // (an object the pool knows is free once the slot lets go)
    const int count = (int)F.list.size();
    for (int k = 0; k < count; ++k) {                                // the commit of cvo_batch_advance_images, with cloud objects handed over instead of written
        const int p = F.list[k];
        own_slot_clouds(b, p);
        if (!b->streams[p].on) fresh_stream(b, p);
        StreamSlot& S = b->streams[p];
        slot_clouds_changed(b, p);
        if (!S.init) {                                                // cvo.cpp:352-360: the first frame only fills the fixed cloud
            S.init = true;
            give_up(b->fixed[p]); b->fixed[p] = F.clouds[k];
            if (!b->moving[p]) b->moving[p].reset(new Cloud());
        } else {
            if (S.has_moving) { give_up(b->fixed[p]); b->fixed[p] = b->moving[p]; b->moving[p].reset(); }   // update_fixed_pcd, cvo.cpp:578-582
            else give_up(b->moving[p]);
            S.has_moving = true;
            b->moving[p] = F.clouds[k];
        }
        if (points_out) points_out[k] = F.points[k];
    }
    stage_taken(b);
    return CVO_OK;
}
int cvo_batch_staged_count(cvo_batch b, int* images, long long* taken) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    return stage_count(b, images, taken);
}
int cvo_batch_get_prev_accum_transform(cvo_batch b, int p, float prev_transform[12], float accum_transform[12]) {
    if (!b || p < 0 || p >= b->max_pairs) return fail(CVO_ERR_INVALID, "bad slot index");
    int rc = batch_settle(b); if (rc) return rc;
    if (!b->streams[p].on) return fail(CVO_ERR_INVALID, "slot is not a stream (cvo_batch_advance_images / cvo_batch_reset_stream)");
    if (prev_transform) std::memcpy(prev_transform, b->streams[p].prev_transform.m, sizeof(float) * 12);
    if (accum_transform) std::memcpy(accum_transform, b->streams[p].accum_transform.m, sizeof(float) * 12);
    return CVO_OK;
}
int cvo_batch_set_num_want(cvo_batch b, int num_want) {
    if (!b || num_want <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    stage_drop(b);                                                  // (frames staged with the old count are not this object's next frames any more)
    b->img.num_want = num_want; return CVO_OK;
}
int cvo_batch_get_cloud(cvo_batch b, int p, int slot, float* xyz, float* feat, int cap, int* n) {
    if (!b || !n || p < 0 || p >= b->max_pairs || (slot != CVO_SLOT_FIXED && slot != CVO_SLOT_MOVING)) return fail(CVO_ERR_INVALID, "bad argument");
    int rc = b->eng.flush_pending(b->eng.stream); if (rc) return rc;   // (clouds handed over by cvo_batch_set_pair(s) are packed by the next launch: here first)
    return download_cloud(b->eng, (slot == CVO_SLOT_FIXED ? b->fixed[p] : b->moving[p]).get(), xyz, feat, cap, n);
}
int cvo_batch_get_selected_points(cvo_batch b, int p, int slot, unsigned short* px, int cap, int* n) {
    if (!b || !n || p < 0 || p >= b->max_pairs || (slot != CVO_SLOT_FIXED && slot != CVO_SLOT_MOVING)) return fail(CVO_ERR_INVALID, "bad argument");
    return download_selected_points(b->eng, (slot == CVO_SLOT_FIXED ? b->fixed[p] : b->moving[p]).get(), px, cap, n);
}

int cvo_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return fail(CVO_ERR_INVALID, "bad argument");
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(CVO_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, ptr, 0) != hipSuccess || d != ptr) {   // the kernels take the caller's own addresses: they must be the device's too
        (void)hipGetLastError(); (void)hipHostUnregister(ptr);
        return fail(CVO_ERR_HIP, "registered memory is not addressable by the device at the caller's address");
    }
    HostRegistry& r = host_registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.ranges.push_back(HostRange{static_cast<const unsigned char*>(ptr), static_cast<const unsigned char*>(ptr) + bytes});
    return CVO_OK;
}
int cvo_host_unregister(void* ptr) {
    if (!ptr) return fail(CVO_ERR_INVALID, "null pointer");
    HostRegistry& r = host_registry();
    {
        std::lock_guard<std::mutex> lk(r.mu);
        auto it = std::find_if(r.ranges.begin(), r.ranges.end(), [&](const HostRange& g) { return g.lo == static_cast<const unsigned char*>(ptr); });
        if (it == r.ranges.end()) return fail(CVO_ERR_INVALID, "not a range cvo_host_register was given");
        r.ranges.erase(it);
    }
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(CVO_ERR_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return CVO_OK;
}
int cvo_batch_set_state(cvo_batch b, int p, const float R[9], const float T[3], float ell) {
    if (!b || p < 0 || p >= b->max_pairs || !R || !T) return fail(CVO_ERR_INVALID, "bad argument");
    int rc = batch_settle(b); if (rc) return rc;
    end_stream(b, p);
    std::memcpy(b->init_states[p].R, R, sizeof(float) * 9); std::memcpy(b->init_states[p].T, T, sizeof(float) * 3);
    b->init_states[p].ell = ell;
    states_dirty(b);
    return CVO_OK;
}
int cvo_batch_set_workgroups(cvo_batch b, int workgroups_per_pair) {
    if (!b || workgroups_per_pair < 0) return fail(CVO_ERR_INVALID, "bad argument");
    b->eng.wg_request = workgroups_per_pair; return CVO_OK;
}
int cvo_batch_set_max_workgroups(cvo_batch b, int max_workgroups) {
    if (!b || max_workgroups < 0) return fail(CVO_ERR_INVALID, "bad argument");
    b->eng.max_wgs = max_workgroups; return CVO_OK;
}
int cvo_batch_set_adoption(cvo_batch b, int on) { if (!b) return fail(CVO_ERR_INVALID, "null batch"); b->eng.adopt = on != 0; return CVO_OK; }
int cvo_batch_set_arith_mode(cvo_batch b, int flags) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (flags & ~CVO_ARITH_EIGEN337) return fail(CVO_ERR_INVALID, "unknown arithmetic mode bit");
    b->eng.arith = flags; return CVO_OK;
}
int cvo_batch_get_arith_mode(cvo_batch b, int* flags) { if (!b || !flags) return fail(CVO_ERR_INVALID, "null argument"); *flags = b->eng.arith; return CVO_OK; }
int cvo_batch_last_adoptions(cvo_batch b, int* pairs_helped) {
    if (!b || !pairs_helped) return fail(CVO_ERR_INVALID, "null argument");
    int rc = b->eng.wait(); if (rc) return rc;
    const PairState* r = b->eng.results(); int n = 0;
    for (int i = 0; i < b->last_n; ++i) n += r[i].joined_at > 0 ? 1 : 0;
    *pairs_helped = n; return CVO_OK;
}
int cvo_batch_last_adoption_retractions(cvo_batch b, int* retractions) {
    if (!b || !retractions) return fail(CVO_ERR_INVALID, "null argument");
    int rc = b->eng.wait(); if (rc) return rc;
    const PairState* r = b->eng.results(); int n = 0;
    for (int i = 0; i < b->last_n; ++i) n += r[i].adopt_retracted;
    *retractions = n; return CVO_OK;
}
int cvo_batch_reset_states(cvo_batch b) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    int rc = batch_settle(b); if (rc) return rc;
    states_dirty(b);                                                  // (stream slots carry their own state: untouched)
    return CVO_OK;
}

int cvo_batch_align_async(cvo_batch b, int n_pairs, void* stream) {
    if (!b || n_pairs <= 0 || n_pairs > b->max_pairs) return fail(CVO_ERR_INVALID, "bad pair count");
    std::vector<int> slots(n_pairs);
    for (int i = 0; i < n_pairs; ++i) slots[i] = i;
    return batch_launch(b, slots.data(), n_pairs, static_cast<hipStream_t>(stream), true);
}
int cvo_batch_align_pairs_async(cvo_batch b, int count, const int* slots, void* stream) {
    if (!b || !slots || count <= 0 || count > b->max_pairs) return fail(CVO_ERR_INVALID, "bad slot list");
    std::vector<unsigned char> seen(b->max_pairs, 0);
    for (int i = 0; i < count; ++i) {
        if (slots[i] < 0 || slots[i] >= b->max_pairs) return fail(CVO_ERR_INVALID, "slot index out of range");
        if (seen[slots[i]]++) return fail(CVO_ERR_INVALID, "slot listed twice");
    }
    return batch_launch(b, slots, count, static_cast<hipStream_t>(stream), false);
}
int cvo_batch_wait(cvo_batch b, cvo_pair_result* results, int n) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    int rc = b->settled ? b->eng.wait() : batch_settle(b); if (rc) return rc;
    if ((rc = stage_place(b, false))) return rc;                     // (frames staged while the launch ran: placed now if their generator has finished too)
    if (results) {
        if (n > b->last_n) return fail(CVO_ERR_INVALID, "more results requested than pairs launched");
        const PairState* r = b->eng.results();
        for (int i = 0; i < n; ++i) {
            std::memcpy(results[i].transform, r[i].transform, sizeof(float) * 12);
            std::memcpy(results[i].R, r[i].R, sizeof(float) * 9); std::memcpy(results[i].T, r[i].T, sizeof(float) * 3);
            results[i].ell = r[i].ell; results[i].iter = r[i].iter; results[i].A_nonzero = r[i].A_nonzero;
            results[i].iterations_run = r[i].iterations_run; results[i].status = r[i].status;
            results[i].rebuilds = r[i].rebuilds; results[i].dense_fallbacks = r[i].dense_fallbacks;
        }
    }
    return CVO_OK;
}
int cvo_batch_done(cvo_batch b, int* done) {
    if (!b || !done) return fail(CVO_ERR_INVALID, "null argument");
    *done = 1;
    if (!b->eng.launched) return CVO_OK;
    HIP_TRY(hipSetDevice(b->eng.device));
    const hipError_t e = hipEventQuery(b->eng.ev1);                 // recorded right behind the launch on its stream
    if (e == hipErrorNotReady) { *done = 0; (void)hipGetLastError(); return CVO_OK; }
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    return CVO_OK;
}
int cvo_batch_last_launch(cvo_batch b, float* kernel_ms, long long* iterations_total, long long* candidates_total) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (kernel_ms) *kernel_ms = b->eng.last_ms;
    long long it = 0, ca = 0;
    const PairState* r = b->eng.results();
    for (int i = 0; i < b->last_n; ++i) { it += r[i].iterations_run; ca += r[i].candidates_total; }
    if (iterations_total) *iterations_total = it;
    if (candidates_total) *candidates_total = ca;
    return CVO_OK;
}
int cvo_batch_last_launch_shape(cvo_batch b, int* grid, int* helpers, int* concurrent) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (grid) *grid = b->eng.last_grid;
    if (helpers) *helpers = b->eng.last_helpers;
    if (concurrent) *concurrent = b->eng.last_concurrent;
    return CVO_OK;
}
int cvo_batch_queue_class(cvo_batch b, int* cls, int* per_class_limit) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    std::lock_guard<std::mutex> lk(adopt_submit_mutex());
    if (cls) *cls = b->eng.queue_class;
    if (per_class_limit) *per_class_limit = hw_queue_count();
    return CVO_OK;
}
int cvo_batch_last_nonzeros(cvo_batch b, long long* nonzeros_total) {
    if (!b || !nonzeros_total) return fail(CVO_ERR_INVALID, "null argument");
    long long nz = 0;
    const PairState* r = b->eng.results();
    for (int i = 0; i < b->last_n; ++i) nz += r[i].nonzeros_total;
    *nonzeros_total = nz;
    return CVO_OK;
}
int cvo_batch_last_pair_seconds(cvo_batch b, int n, double* seconds) {
    if (!b || !seconds || n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "bad argument");
    const PairState* r = b->eng.results();
    for (int i = 0; i < n; ++i) seconds[i] = 1e-8 * (double)r[i].clk_ticks;      // 100 MHz ticks workgroup 0 spent on the pair
    return CVO_OK;
}
int cvo_batch_last_pair_spans(cvo_batch b, int n, double* start_s, double* end_s, int* joined_at) {
    if (!b || !start_s || !end_s || n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "bad argument");
    const PairState* r = b->eng.results();
    for (int i = 0; i < n; ++i) {
        start_s[i] = 1e-8 * (double)r[i].clk_t0; end_s[i] = 1e-8 * (double)(r[i].clk_t0 + r[i].clk_ticks);
        if (joined_at) joined_at[i] = r[i].joined_at;
    }
    return CVO_OK;
}
int cvo_batch_last_tail_seconds(cvo_batch b, double seconds[4]) {
    if (!b || !seconds) return fail(CVO_ERR_INVALID, "null argument");
    const PairState* r = b->eng.results();
    for (int q = 0; q < 4; ++q) { seconds[q] = 0; for (int i = 0; i < b->last_n; ++i) seconds[q] += 1e-8 * (double)r[i].tail_ticks[q]; }
    return CVO_OK;
}
int cvo_batch_last_cull_masks(cvo_batch b, int n, unsigned long long* masks, unsigned long long* predicted) {
    if (!b || !masks || n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "bad argument");
    const PairState* r = b->eng.results();
    for (int i = 0; i < n; ++i) { masks[i] = r[i].cull_mask; if (predicted) predicted[i] = r[i].predict_mask; }
    return CVO_OK;
}
int cvo_batch_last_phase_seconds(cvo_batch b, double seconds[10]) {
    if (!b || !seconds) return fail(CVO_ERR_INVALID, "null argument");
    const PairState* r = b->eng.results();
    for (int q = 0; q < 10; ++q) seconds[q] = 0;
    for (int i = 0; i < b->last_n; ++i) for (int q = 0; q < 10; ++q) seconds[q] += 1e-8 * (double)r[i].phase_ticks[q];
    {   // slot 9 doubles as the measured shader clock in GHz (cycles per 100 MHz tick), averaged over pairs
        double cyc = 0, tk = 0;
        for (int i = 0; i < b->last_n; ++i) { cyc += (double)r[i].clk_cycles; tk += (double)r[i].clk_ticks; }
        if (std::getenv("CVO_HIP_REPORT_CLOCK") && tk > 0) std::fprintf(stderr, "[cvo_hip] shader clock %.3f GHz\n", cyc / tk * 0.1);
    }
    return CVO_OK;
}
int cvo_batch_compute_innerproduct_lc(cvo_batch b, int n, const float* prior_tran, const float* lc_prior_tran, const float* lc_prior_tran_2,
                                      cvo_lc_scores* out) {
    if (!b || !prior_tran || !lc_prior_tran || !lc_prior_tran_2 || !out) return fail(CVO_ERR_INVALID, "null argument");
    if (n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "more pairs than the last launch aligned");
    int rc = check_last_clouds(b); if (rc) return rc;
    rc = b->settled ? b->eng.wait() : batch_settle(b); if (rc) return rc;
    const PairState* res = b->eng.results();
    std::vector<Engine::ScoreReq> rq((size_t)n * 8);
    for (int i = 0; i < n; ++i) {
        const int p = b->last_slots[i];
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "compute_innerproduct_lc: empty cloud in the batch");
        const float* lc_tran = res[i].transform;                     // lc_post = result.transform, keyframe_graph.cpp:702
        const float ell = res[i].ell;                                // the ell align() left behind (Q1), cvo.cpp:395
        Engine::ScoreReq* q = &rq[(size_t)i * 8];
        q[0] = {mv, prior_tran + 12 * i, fx, false, ell};            // cvo.cpp:539
        q[1] = {mv, lc_prior_tran + 12 * i, fx, false, ell};         // cvo.cpp:541
        q[2] = {mv, nullptr, fx, false, ell};                        // cvo.cpp:543
        q[3] = {mv, lc_tran, fx, false, ell};                        // cvo.cpp:545
        q[4] = {fx, nullptr, fx, false, ell};                        // cvo.cpp:550
        q[5] = {mv, nullptr, mv, false, ell};                        // cvo.cpp:551
        q[6] = {mv, lc_tran, fx, true, ell};                         // cvo.cpp:555
        q[7] = {mv, lc_prior_tran_2 + 12 * i, fx, true, ell};        // cvo.cpp:558
    }
    std::vector<double> r((size_t)n * 8 * 24);
    rc = b->eng.score_many(rq.data(), n * 8, reinterpret_cast<double (*)[24]>(r.data())); if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const double (*ri)[24] = reinterpret_cast<const double (*)[24]>(r.data() + (size_t)i * 8 * 24);
        cvo_lc_scores& o = out[i];
        finish_inn_p(ri[0], &o.inn_prior); finish_inn_p(ri[1], &o.inn_lc_prior); finish_inn_p(ri[2], &o.inn_pre); finish_inn_p(ri[3], &o.inn_post);
        finish_inn_p(ri[4], &o.inn_fixed_pcd); finish_inn_p(ri[5], &o.inn_moving_pcd);
        o.cos_angle = o.inn_post.value / (sqrtf(o.inn_fixed_pcd.value) * sqrtf(o.inn_moving_pcd.value));   // cvo.cpp:552
        o.inliers_svd = (int)ri[6][1];
        finish_hessian(ri[6] + 2, o.inliers_svd, o.post_hessian);
        o.inliers_pnpransac = (int)ri[7][1];
        const bool reject = (o.inn_post.value <= o.inn_pre.value) || (o.inn_post.value <= o.inn_lc_prior.value) ||
                            (o.inn_post.value <= o.inn_prior.value) || o.cos_angle < 0.1f;          // keyframe_graph.cpp:711-712
        o.accept = reject ? 0 : 1;
    }
    return CVO_OK;
}
// The tracker's score block (cvo.cpp:475-503) for every pair of the last launch, each with its own align() result as `tran` and
// the ell that align() left behind (Q1).  enqueue: one launch behind the align launch on its stream, transforms read from the
// device-resident states, nothing waits; results: waits and finishes the sums on the host.
int cvo_batch_enqueue_innerproduct(cvo_batch b, int n) {
    if (!b) return fail(CVO_ERR_INVALID, "null argument");
    if (n <= 0 || n > b->last_n || !b->eng.launched) return fail(CVO_ERR_INVALID, "more pairs than the last launch aligned");
    int rc = check_last_clouds(b); if (rc) return rc;
    std::vector<Engine::ScoreReq> rq((size_t)n * 5);
    for (int i = 0; i < n; ++i) {
        const int p = b->last_slots[i];                              // (its device state: the slot's, Engine::launch's state_index)
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "compute_innerproduct: empty cloud in the batch");
        Engine::ScoreReq* q = &rq[(size_t)i * 5];
        q[0] = {mv, nullptr, fx, false, 0.f, p, false};              // cvo.cpp:489
        q[1] = {mv, nullptr, fx, false, 0.f, p, true};               // cvo.cpp:491
        q[2] = {fx, nullptr, fx, false, 0.f, p, false};              // cvo.cpp:496
        q[3] = {mv, nullptr, mv, false, 0.f, p, false};              // cvo.cpp:497
        q[4] = {mv, nullptr, fx, true, 0.f, p, true};                // cvo.cpp:500
    }
    return b->eng.score_enqueue(rq.data(), n * 5, b->eng.last_stream);
}
int cvo_batch_set_tail_scores(cvo_batch b, int on) { if (!b) return fail(CVO_ERR_INVALID, "null batch"); b->eng.tail_scores = on != 0; return CVO_OK; }
namespace {
// the score blocks the last launch answered in its tail; whatever a pair's workgroup could not answer (PairDesc::score_out[23]) is
// computed by the score kernel now, all missing requests of the batch in one launch
int collect_tail_scores(cvo_batch b, int n, double* r /* n x 5 x 24 */) {
    if (n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "more pairs than the last launch aligned");
    int rc = check_last_clouds(b); if (rc) return rc;
    rc = b->settled ? b->eng.wait() : batch_settle(b); if (rc) return rc;
    std::memcpy(r, b->eng.h_tail.p, sizeof(double) * (size_t)n * 5 * 24);
    static const int bit_of[5] = {TAIL_PRE, TAIL_POST, TAIL_FIXED, TAIL_MOVING, TAIL_HESSIAN};
    std::vector<Engine::ScoreReq> rq; std::vector<int> where;
    for (int i = 0; i < n; ++i) {
        const int mask = (int)r[(size_t)i * 120 + 23];
        const int p = b->last_slots[i];
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        const Engine::ScoreReq all[5] = {{mv, nullptr, fx, false, 0.f, p, false}, {mv, nullptr, fx, false, 0.f, p, true}, {fx, nullptr, fx, false, 0.f, p, false},
                                         {mv, nullptr, mv, false, 0.f, p, false}, {mv, nullptr, fx, true, 0.f, p, true}};   // cvo.cpp:489, 491, 496, 497, 500
        for (int q = 0; q < 5; ++q) if (!(mask & bit_of[q])) { rq.push_back(all[q]); where.push_back(i * 5 + q); }
    }
    if (!rq.empty()) {
        std::vector<double> extra(rq.size() * 24);
        rc = b->eng.score_many(rq.data(), (int)rq.size(), reinterpret_cast<double (*)[24]>(extra.data())); if (rc) return rc;
        for (size_t k = 0; k < rq.size(); ++k) std::memcpy(r + (size_t)where[k] * 24, extra.data() + k * 24, sizeof(double) * 24);
    }
    for (int i = 0; i < n; ++i) r[(size_t)i * 120 + 23] = 0.0;
    return CVO_OK;
}
}  // namespace
namespace {
// the sums of one pair's score block (5 requests x 24 doubles) -> cvo_track_scores
void finish_track_scores(const double (*ri)[24], cvo_track_scores& o) {
    finish_inn_p(ri[0], &o.inn_pre); finish_inn_p(ri[1], &o.inn_post); finish_inn_p(ri[2], &o.inn_fixed_pcd); finish_inn_p(ri[3], &o.inn_moving_pcd);
    o.cos_angle = o.inn_post.value / (sqrtf(o.inn_fixed_pcd.value) * sqrtf(o.inn_moving_pcd.value));           // cvo.cpp:498
    o.inliers = (int)ri[4][1];                                   // cvo.cpp:708 with the caller's counter starting at 0 (local_tracker.cpp:240)
    finish_hessian(ri[4] + 2, o.inliers, o.post_hessian);
}
}  // namespace
int cvo_batch_last_tail_answers(cvo_batch b, int n, int* masks) {
    if (!b || !masks || n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "bad argument");
    int rc = b->eng.wait(); if (rc) return rc;
    for (int i = 0; i < n; ++i) masks[i] = b->eng.last_tail ? (int)static_cast<const double*>(b->eng.h_tail.p)[(size_t)i * 120 + 23] : 0;
    return CVO_OK;
}
int cvo_batch_innerproduct_results(cvo_batch b, int n, cvo_track_scores* out) {
    if (!b || !out) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<double> r((size_t)std::max(n, 1) * 5 * 24);
    int rc = (b->eng.last_tail && b->eng.score_pending == 0) ? collect_tail_scores(b, n, r.data())
                                                             : b->eng.score_collect(n * 5, reinterpret_cast<double (*)[24]>(r.data()));
    if (rc) return rc;
    for (int i = 0; i < n; ++i) finish_track_scores(reinterpret_cast<const double (*)[24]>(r.data() + (size_t)i * 5 * 24), out[i]);
    return CVO_OK;
}
int cvo_batch_compute_innerproduct(cvo_batch b, int n, cvo_track_scores* out) {
    int rc = cvo_batch_enqueue_innerproduct(b, n); if (rc) return rc;
    return cvo_batch_innerproduct_results(b, n, out);
}
// ---- per-point support and point matches of a batch's last launch (include/cvo_hip.h, "per-point support", "point matches")
extern "C++" {                                                        // (the helpers below have templates among them)
namespace {
// Positions of b's last launch (pairs null: 0 .. count-1), none twice: each(k, slot) for the k-th listed one, in order, as soon as it has been checked.
template <class Each>
int last_launch_pairs(cvo_batch b, int count, const int* pairs, const std::string& what, Each&& each) {
    if (!b->eng.launched || count <= 0 || count > b->last_n) return fail(CVO_ERR_INVALID, "more pairs than the last launch aligned");
    int rc = check_last_clouds(b); if (rc) return rc;
    std::vector<unsigned char> seen(b->last_n, 0);
    for (int k = 0; k < count; ++k) {
        const int i = pairs ? pairs[k] : k;
        if (i < 0 || i >= b->last_n) return fail(CVO_ERR_INVALID, what + ": pair " + std::to_string(i) + " is not a position of the last launch");
        if (seen[i]++) return fail(CVO_ERR_INVALID, what + ": pair " + std::to_string(i) + " listed twice");
        if ((rc = each(k, b->last_slots[i]))) return rc;
    }
    return CVO_OK;
}
// The device form's arrays: every one that is given is aligned and memory the device can write (the rule of cvo_device_cloud: check_device_plane)
struct DstArray { const void* p; long long bytes; const char* name; unsigned align; };
int check_dst_arrays(int device, const DstArray* arr, int n, const std::string& who) {
    for (int q = 0; q < n; ++q) {
        const DstArray& x = arr[q];
        if (!x.p) continue;
        if (reinterpret_cast<uintptr_t>(x.p) & (x.align - 1u)) return fail(CVO_ERR_INVALID, who + x.name + " is not " + std::to_string(x.align) + "-byte aligned");
        int rc = check_device_plane(device, x.p, x.bytes, x.bytes, 1, who + x.name, "array"); if (rc) return rc;
    }
    return CVO_OK;
}
// One pair's record of a point-support call: both directions' arrays, each direction whole or absent; on_device: every array is n x 4 bytes.
// Nothing is queued here.
int check_dst(int device, const cvo_point_support_dst& d, int n_moving, int n_fixed, bool on_device, const std::string& who) {
    if (!d.sum_moving != !d.count_moving || !d.sum_fixed != !d.count_fixed) return fail(CVO_ERR_INVALID, who + "a direction needs its sum and its count array");
    if (!d.sum_moving && !d.sum_fixed) return fail(CVO_ERR_INVALID, who + "no output array");
    const DstArray arr[4] = {{d.sum_moving, 4ll * n_moving, "sum_moving", 4}, {d.count_moving, 4ll * n_moving, "count_moving", 4},
                             {d.sum_fixed, 4ll * n_fixed, "sum_fixed", 4}, {d.count_fixed, 4ll * n_fixed, "count_fixed", 4}};
    return on_device ? check_dst_arrays(device, arr, 4, who) : CVO_OK;
}
// One pair's record of a point-matches call: a direction's five arrays all given or all absent, not both absent; on_device: fit is two records,
// 8-byte aligned.  Nothing is queued here.
int check_dst(int device, const cvo_point_matches_dst& d, int n_moving, int n_fixed, bool on_device, const std::string& who) {
    const DstArray arr[11] = {
        {d.best_moving, 4ll * n_moving, "best_moving", 4}, {d.best_value_moving, 4ll * n_moving, "best_value_moving", 4}, {d.mean_moving, 12ll * n_moving, "mean_moving", 4},
        {d.sum_moving, 4ll * n_moving, "sum_moving", 4}, {d.count_moving, 4ll * n_moving, "count_moving", 4},
        {d.best_fixed, 4ll * n_fixed, "best_fixed", 4}, {d.best_value_fixed, 4ll * n_fixed, "best_value_fixed", 4}, {d.mean_fixed, 12ll * n_fixed, "mean_fixed", 4},
        {d.sum_fixed, 4ll * n_fixed, "sum_fixed", 4}, {d.count_fixed, 4ll * n_fixed, "count_fixed", 4},
        {d.fit, 2ll * sizeof(cvo_match_fit), "fit", 8}};
    for (int side = 0; side < 2; ++side) {
        int given = 0;
        for (int q = 0; q < 5; ++q) given += arr[5 * side + q].p ? 1 : 0;
        if (given != 0 && given != 5) return fail(CVO_ERR_INVALID, who + "a direction needs all five of its arrays");
    }
    if (!d.best_moving && !d.best_fixed) return fail(CVO_ERR_INVALID, who + "no output array");
    return on_device ? check_dst_arrays(device, arr, 11, who) : CVO_OK;
}
// The requests of the listed slots of b (their device states name transform and ell), checked; then one launch on the stream of b's last launch.
// what: "point support" / "point matches", as the messages name the call.
template <class Dst>
int batch_sides_run(cvo_batch b, const std::vector<int>& slots, const Dst* dst, bool on_device, void* out_stream, const std::string& what) {
    Engine& E = b->eng;
    if (on_device) HIP_TRY(hipSetDevice(E.device));
    std::vector<Engine::SideReq<Dst>> rq(slots.size());
    for (size_t k = 0; k < slots.size(); ++k) {
        const int p = slots[k];
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, what + ": empty cloud in the batch");
        int rc = check_dst(E.device, dst[k], mv->n, fx->n, on_device, what + ", record " + std::to_string(k) + ": "); if (rc) return rc;
        rq[k] = Engine::SideReq<Dst>{mv, nullptr, fx, 0.f, p, true, dst[k]};
    }
    return E.point_sides(rq.data(), (int)rq.size(), E.last_stream, !on_device, on_device ? static_cast<hipStream_t>(out_stream) : nullptr);
}
template <class Dst>
int batch_sides(cvo_batch b, int count, const int* pairs, const Dst* dst, bool on_device, void* out_stream, const std::string& what) {
    if (!b || !dst) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<int> slots;
    int rc = last_launch_pairs(b, count, pairs, what, [&](int k, int slot) { if (k == 0) slots.reserve(count); slots.push_back(slot); return (int)CVO_OK; }); if (rc) return rc;
    return batch_sides_run(b, slots, dst, on_device, out_stream, what);
}
}  // namespace
}  // extern "C++"
int cvo_batch_point_support(cvo_batch b, int count, const int* pairs, const cvo_point_support_dst* dst) { return batch_sides(b, count, pairs, dst, false, nullptr, "point support"); }
int cvo_batch_point_support_device(cvo_batch b, int count, const int* pairs, const cvo_point_support_dst* dst, void* out_stream) {
    return batch_sides(b, count, pairs, dst, true, out_stream, "point support");
}
int cvo_point_matches(cvo_handle h, int slot_a, const float* tran_a, int slot_b, const cvo_point_matches_dst* dst, int cap_a, int cap_b) {
    if (!h || !dst) return fail(CVO_ERR_INVALID, "null argument");
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    int rc = check_dst(h->eng.device, *dst, a ? a->n : 0, b ? b->n : 0, false, "point matches: "); if (rc) return rc;
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "point matches: empty cloud slot");
    if ((dst->best_moving && cap_a < a->n) || (dst->best_fixed && cap_b < b->n)) return fail(CVO_ERR_INVALID, "point matches: an output array is shorter than its cloud");
    const Engine::MatchReq rq[1] = {{a, tran_a, b, h->ell, -1, false, *dst}};
    return h->eng.point_sides(rq, 1, h->eng.stream, true);
}
int cvo_batch_point_matches(cvo_batch b, int count, const int* pairs, const cvo_point_matches_dst* dst) { return batch_sides(b, count, pairs, dst, false, nullptr, "point matches"); }
int cvo_batch_point_matches_device(cvo_batch b, int count, const int* pairs, const cvo_point_matches_dst* dst, void* out_stream) {
    return batch_sides(b, count, pairs, dst, true, out_stream, "point matches");
}
int cvo_batch_results_to_device(cvo_batch b, void* dst_device, int n, void* stream) {
    if (!b || !dst_device || n <= 0 || n > b->last_n) return fail(CVO_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(b->eng.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->eng.last_stream;
    hipError_t e = launch_copy_records(static_cast<const float*>(b->eng.d_records.p), static_cast<float*>(dst_device), n, s);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("record copy kernel launch: ") + hipGetErrorString(e));
    return CVO_OK;
}
int cvo_batch_result_records(cvo_batch b, const void** records_device) {
    if (!b || !records_device) return fail(CVO_ERR_INVALID, "null argument");
    if (!b->eng.launched) return fail(CVO_ERR_INVALID, "no launch yet");
    *records_device = b->eng.d_records.p;
    return CVO_OK;
}

// ======================= K-stream tracker steps (cvo_tracks_*): the two cvo::cvo objects of local_tracker, K streams per call ===========
// A stream is the pair of objects local_tracker owns (local_tracker.cpp:228-251, 330-338, 356-431, 506): slot s of the batch `odo` is its
// cvo_odometry (a stream slot, as cvo_batch_advance_images keeps it), slot s of the batch `key` holds the fixed and moving cloud of its
// cvo_keyframe and that object's device state; what a keyframe object carries between frames lives in KeyObject on the host, as a handle
// carries it.  A frame is generated once into a cloud object of its own; the slots that hold it share ownership (up to four at once: the
// odometry moving / fixed cloud, the keyframe moving / previous / fixed cloud), and a cloud object is only written again when nobody holds it.
struct KeyObject {
    bool pre_pc_init = false, first_frame = true;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0}, ell = 0.f;
    int iter = 0, A_nonzero = 0;
    Aff transform = aff_identity(), prev_transform = aff_identity(), accum_transform = aff_identity();
    std::shared_ptr<Cloud> previous;        // ptr_previous_pcd (fixed and moving: the key batch's slot)
};
struct TrackStream {
    int frames = 0;                         // frames seen: the next step's phase is min(frames, 2)
    bool commit_pending = false;            // a phase-2 frame has been waited for and the caller's decision is not in yet
    Aff t_odometry = aff_identity();        // the odometry transform of that frame (reset_keyframe's argument)
    KeyObject key;
};
struct cvo_tracks_s {
    cvo_params prm;
    int max_streams = 0;
    cvo_batch odo = nullptr, key = nullptr;
    std::vector<TrackStream> st;
    std::vector<std::shared_ptr<Cloud>> pool;   // every cloud object made so far; one that only the pool holds is free
    PinBuf h_link_in, h_link_out;
    // the step in flight
    bool in_flight = false;
    std::vector<int> list, phase, points, odo_pos, key_pos;   // per listed stream: its phase, points, and position in the two launches (-1: not in it)
    std::vector<std::shared_ptr<Cloud>> moving_before;          // the keyframe object's moving cloud before the step (put back when the odometry alignment fails)
    int n_odo = 0, n_key = 0;
    // the step waited for last, until the next commit or step: which objects of its listed streams aligned with CVO_OK (cvo_tracks_point_support)
    bool support_valid = false;
    std::vector<unsigned char> odo_ok, key_ok;
};

namespace {
void tracks_free_cloud(cvo_tracks_s* t, std::shared_ptr<Cloud>& out) { pool_free_cloud(t->pool, out); }
void tracks_fresh_stream(cvo_tracks_s* t, int s) {
    t->odo->fixed[s].reset(); t->odo->moving[s].reset(); t->key->fixed[s].reset(); t->key->moving[s].reset();
    fresh_stream(t->odo, s);
    t->st[s] = TrackStream();
    t->st[s].key.ell = t->prm.ell;
}
void pair_result_from(const PairState& r, cvo_pair_result& o) {
    std::memcpy(o.transform, r.transform, sizeof(float) * 12);
    std::memcpy(o.R, r.R, sizeof(float) * 9); std::memcpy(o.T, r.T, sizeof(float) * 3);
    o.ell = r.ell; o.iter = r.iter; o.A_nonzero = r.A_nonzero; o.iterations_run = r.iterations_run; o.status = r.status;
    o.rebuilds = r.rebuilds; o.dense_fallbacks = r.dense_fallbacks;
}
// The score blocks of the positions of b's last launch marked in `want` (cvo.cpp:475-503, tran = the alignment's own result): what the launch
// answered in its tail is taken from there, the rest goes to the score kernel in one launch (as cvo_batch_innerproduct_results has it).
// out: one entry per position; positions not wanted are left alone.
int tracks_scores(cvo_batch b, int n, const std::vector<unsigned char>& want, std::vector<cvo_track_scores>& out) {
    std::vector<double> r((size_t)std::max(n, 1) * 5 * 24, 0.0);
    if (b->eng.last_tail) std::memcpy(r.data(), b->eng.h_tail.p, sizeof(double) * (size_t)n * 5 * 24);
    static const int bit_of[5] = {TAIL_PRE, TAIL_POST, TAIL_FIXED, TAIL_MOVING, TAIL_HESSIAN};
    std::vector<Engine::ScoreReq> rq; std::vector<int> where;
    for (int i = 0; i < n; ++i) {
        if (!want[i]) continue;
        const int mask = b->eng.last_tail ? (int)r[(size_t)i * 120 + 23] : 0;
        const int p = b->last_slots[i];
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        const Engine::ScoreReq all[5] = {{mv, nullptr, fx, false, 0.f, p, false}, {mv, nullptr, fx, false, 0.f, p, true}, {fx, nullptr, fx, false, 0.f, p, false},
                                         {mv, nullptr, mv, false, 0.f, p, false}, {mv, nullptr, fx, true, 0.f, p, true}};   // cvo.cpp:489, 491, 496, 497, 500
        for (int q = 0; q < 5; ++q) if (!(mask & bit_of[q])) { rq.push_back(all[q]); where.push_back(i * 5 + q); }
    }
    if (!rq.empty()) {
        std::vector<double> extra(rq.size() * 24);
        int rc = b->eng.score_many(rq.data(), (int)rq.size(), reinterpret_cast<double (*)[24]>(extra.data())); if (rc) return rc;
        for (size_t k = 0; k < rq.size(); ++k) std::memcpy(r.data() + (size_t)where[k] * 24, extra.data() + k * 24, sizeof(double) * 24);
    }
    for (int i = 0; i < n; ++i) {
        if (!want[i]) continue;
        r[(size_t)i * 120 + 23] = 0.0;
        finish_track_scores(reinterpret_cast<const double (*)[24]>(r.data() + (size_t)i * 5 * 24), out[i]);
    }
    return CVO_OK;
}
int tracks_check_list(cvo_tracks_s* t, int count, const int* streams) {
    if (!t || count <= 0 || count > t->max_streams) return fail(CVO_ERR_INVALID, "bad stream count");
    if (!streams) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<unsigned char> seen(t->max_streams, 0);
    for (int k = 0; k < count; ++k) {
        if (streams[k] < 0 || streams[k] >= t->max_streams) return fail(CVO_ERR_INVALID, "stream index out of range");
        if (seen[streams[k]]++) return fail(CVO_ERR_INVALID, "stream listed twice");
    }
    return CVO_OK;
}
}  // namespace

int cvo_tracks_create(const cvo_params* p, int device, int max_streams, cvo_tracks* out) {
    if (!out || max_streams <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    *out = nullptr;
    std::unique_ptr<cvo_tracks_s> t(new cvo_tracks_s());
    if (p) t->prm = *p; else cvo_default_params(&t->prm);
    t->max_streams = max_streams;
    int rc = batch_create(&t->prm, device, max_streams, &t->odo, false); if (rc) return rc;
    rc = batch_create(&t->prm, device, max_streams, &t->key, false);
    // the keyframe launch starts from device states the link kernel writes before that launch has sized the table: sized here, once
    if (!rc) rc = t->key->eng.d_states.ensure(sizeof(PairState) * (size_t)max_streams);
    if (rc) { cvo_batch_destroy(t->odo); cvo_batch_destroy(t->key); return rc; }
    for (cvo_batch b : {t->odo, t->key}) { b->eng.tail_scores = true; b->eng.queue_behind = true; }
    t->odo->stage.pool = &t->pool;                                   // staged frames (cvo_tracks_stage_async) go into cloud objects of the streams' pool
    t->st.resize(max_streams);
    for (int s = 0; s < max_streams; ++s) tracks_fresh_stream(t.get(), s);
    *out = t.release();
    return CVO_OK;
}
int cvo_tracks_destroy(cvo_tracks t) {
    if (!t) return CVO_OK;
    (void)hipSetDevice(t->odo->eng.device);
    if (t->odo->eng.launched && t->odo->eng.last_stream) (void)hipStreamSynchronize(t->odo->eng.last_stream);
    if (t->key->eng.launched && t->key->eng.last_stream) (void)hipStreamSynchronize(t->key->eng.last_stream);
    stage_destroy(t->odo);                                           // (drains the stage stream; its clouds return to the pool)
    for (TrackStream& s : t->st) s.key.previous.reset();
    t->moving_before.clear();
    report_step_laps("tracks");
    cvo_batch_destroy(t->odo); cvo_batch_destroy(t->key);
    t->pool.clear();
    t->h_link_in.release(); t->h_link_out.release();
    delete t;
    return CVO_OK;
}
int cvo_tracks_set_num_want(cvo_tracks t, int num_want) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    return cvo_batch_set_num_want(t->odo, num_want);
}
int cvo_tracks_set_arith_mode(cvo_tracks t, int flags) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    int rc = cvo_batch_set_arith_mode(t->odo, flags); if (rc) return rc;
    return cvo_batch_set_arith_mode(t->key, flags);
}
int cvo_tracks_reset(cvo_tracks t, int s) {
    if (!t || s < 0 || s >= t->max_streams) return fail(CVO_ERR_INVALID, "bad stream index");
    if (t->in_flight) return fail(CVO_ERR_INVALID, "a step is in flight (cvo_tracks_wait first)");
    tracks_fresh_stream(t, s);
    t->support_valid = false;
    return CVO_OK;
}
namespace {
// what a step checks about its arguments (a stage call checks the same)
int tracks_check_images(cvo_tracks_s* t, int count, const int* streams, const ImageSrc& src, int width, int height,
                        const cvo_camera* cams, const int* cam_index) {
    int rc = tracks_check_list(t, count, streams); if (rc) return rc;
    if ((!src.dev && (!src.bgr8 || !src.depth16)) || !cams) return fail(CVO_ERR_INVALID, "null argument");
    if (!image_size_ok(width, height)) return fail(CVO_ERR_INVALID, "image size out of range");
    for (int k = 0; k < count; ++k) {
        if (!src.dev && (!src.bgr8[k] || !src.depth16[k])) return fail(CVO_ERR_INVALID, "null image pointer");
        if (cam_index && cam_index[k] < 0) return fail(CVO_ERR_INVALID, "camera index out of range");
    }
    return CVO_OK;
}
// ... and what depends on the streams' state
int tracks_check_state(cvo_tracks_s* t, int count, const int* streams) {
    if (t->in_flight) return fail(CVO_ERR_INVALID, "a step is in flight (cvo_tracks_wait first)");
    for (int k = 0; k < count; ++k)
        if (t->st[streams[k]].commit_pending) return fail(CVO_ERR_INVALID, "stream " + std::to_string(streams[k]) + " waits for the decision on its last frame (cvo_tracks_commit)");
    return CVO_OK;
}
// The step once its frames' point counts are known.  staged (null: generated by this call, records R): the frames' finished cloud objects, handed to the
// slots as they are; else every frame is scattered into a cloud object nobody holds.  Then the launches.
int tracks_step_run(cvo_tracks_s* t, int count, const int* streams, const int* npts, const std::vector<std::shared_ptr<Cloud>>* staged, const PcdImgRec* R, void* hip_stream) {
    cvo_batch bo = t->odo, bk = t->key;
    int rc;
    // every frame into a cloud object nobody holds; the objects' slots take it (local_tracker.cpp:228-231, 233, 356, 415; update_fixed_pcd :403)
    t->support_valid = false;
    t->list.assign(streams, streams + count);
    t->phase.assign(count, 0); t->points.assign(count, 0); t->odo_pos.assign(count, -1); t->key_pos.assign(count, -1);
    t->moving_before.assign(count, nullptr);
    std::vector<Cloud*> dst(count); std::vector<int> img(count), slots_odo, slots_key;
    for (int k = 0; k < count; ++k) {
        const int s = streams[k];
        TrackStream& S = t->st[s]; StreamSlot& O = bo->streams[s];
        std::shared_ptr<Cloud> c;
        if (staged) c = (*staged)[k]; else tracks_free_cloud(t, c);
        dst[k] = c.get(); img[k] = k;
        const int ph = std::min(S.frames, 2);
        t->phase[k] = ph; t->points[k] = npts[k];
        if (ph == 0) {                                               // both objects' set_pcd of the first frame: their FIXED cloud (cvo.cpp:352-360)
            bo->fixed[s] = c; bk->fixed[s] = c; O.init = true;
        } else {
            if (O.has_moving) bo->fixed[s] = bo->moving[s];          // update_fixed_pcd
            bo->moving[s] = c; O.has_moving = true;
            t->odo_pos[k] = (int)slots_odo.size(); slots_odo.push_back(s);
            if (ph == 2) {                                           // the keyframe object's match_keyframe of the same frame
                t->moving_before[k] = bk->moving[s]; bk->moving[s] = c;
                t->key_pos[k] = (int)slots_key.size(); slots_key.push_back(s);
            }
        }
        ++S.frames;
    }
    t->n_odo = (int)slots_odo.size(); t->n_key = (int)slots_key.size();
    if (!staged) { Lap lap(StepLaps::SCATTER); if ((rc = batch_scatter(bo, dst, img, R))) return rc; }
    Lap lap(StepLaps::LAUNCH);
    ++step_laps()->steps;
    if (t->n_odo == 0) { t->in_flight = true; return CVO_OK; }
    // ONE odometry launch over the listed streams that align; its tail answers the score blocks
    if ((rc = batch_launch(bo, slots_odo.data(), t->n_odo, static_cast<hipStream_t>(hip_stream), false))) return rc;
    t->in_flight = true;                                             // (from here on there is something to wait for)
    if (t->n_key == 0) return CVO_OK;
    const hipStream_t hs = bo->eng.last_stream;
    // the link: reset_initial on the device, from the odometry launch's device states into the keyframe launch's
    if ((rc = t->h_link_in.ensure(sizeof(TrackLinkIn) * (size_t)t->max_streams)) || (rc = t->h_link_out.ensure(sizeof(TrackLinkOut) * (size_t)t->max_streams))) return rc;
    TrackLinkIn* li = static_cast<TrackLinkIn*>(t->h_link_in.p);
    for (int i = 0; i < t->n_key; ++i) {
        const int s = slots_key[i]; const KeyObject& K = t->st[s].key;
        std::memcpy(li[i].R, K.R, sizeof(K.R)); std::memcpy(li[i].T, K.T, sizeof(K.T)); li[i].ell = K.ell;
        std::memcpy(li[i].transform, K.transform.m, sizeof(li[i].transform));
        li[i].iter = K.iter; li[i].odo_state = s; li[i].key_state = s; li[i].pad_ = 0;
        bk->streams[s] = StreamSlot(); bk->dirty[s] = 0;             // a plain pair that starts from its device state (Engine::launch: upload_each = 0)
    }
    const hipError_t e = launch_track_link(li, static_cast<const PairState*>(bo->eng.d_states.p), static_cast<PairState*>(bk->eng.d_states.p),
                                           static_cast<TrackLinkOut*>(t->h_link_out.p), t->n_key, hs);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("track link kernel launch: ") + hipGetErrorString(e));
    // ONE keyframe launch over the phase-2 streams, behind the link kernel on the same stream
    return batch_launch(bk, slots_key.data(), t->n_key, hs, false);
}
int tracks_step_from(cvo_tracks_s* t, int count, const int* streams, const ImageSrc& src, int width, int height,
                     const cvo_camera* cams, const int* cam_index, void* hip_stream) {
    int rc = tracks_check_images(t, count, streams, src, width, height, cams, cam_index); if (rc) return rc;
    if ((rc = tracks_check_state(t, count, streams))) return rc;
    cvo_batch bo = t->odo, bk = t->key;
    if ((rc = batch_settle(bo)) || (rc = batch_settle(bk))) return rc;
    std::vector<cvo_camera> cam_of(count);
    for (int k = 0; k < count; ++k) cam_of[k] = cams[cam_index ? cam_index[k] : 0];
    const PcdImgRec* R = nullptr;
    if ((rc = batch_generate(bo, count, src, width, height, nullptr, cam_of.data(), &R))) return rc;   // (the step's one host sync; fails before any stream changes)
    std::vector<int> npts(count);
    for (int k = 0; k < count; ++k) npts[k] = R[k].npts;
    return tracks_step_run(t, count, streams, npts.data(), nullptr, R, hip_stream);
}
}  // namespace
int cvo_tracks_step_async(cvo_tracks t, int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                          const cvo_camera* cams, const int* cam_index, void* hip_stream) {
    return tracks_step_from(t, count, streams, ImageSrc::host(bgr8, depth16), width, height, cams, cam_index, hip_stream);
}
int cvo_tracks_step_device_async(cvo_tracks t, int count, const int* streams, const cvo_device_image* images, int width, int height,
                                 const cvo_camera* cams, const int* cam_index, void* hip_stream, void* image_stream) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    int rc = check_device_images(t->odo->eng.device, count, images, width, height); if (rc) return rc;
    return tracks_step_from(t, count, streams, ImageSrc::device(images, image_stream), width, height, cams, cam_index, hip_stream);
}
// The cloud twin (see cvo_device_cloud): the step's frames as clouds in caller-owned device memory, each ingested once into a cloud object both of the
// stream's objects hold; phases, commit protocol and stage are cvo_tracks_step_async's.  A refused call changes no stream and keeps the stage.
int cvo_tracks_step_device_clouds_async(cvo_tracks t, int count, const int* streams, const cvo_device_cloud* clouds, void* hip_stream, void* cloud_stream) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    int rc = check_device_clouds(t->odo->eng.device, count, clouds); if (rc) return rc;
    if ((rc = tracks_check_list(t, count, streams))) return rc;
    if ((rc = tracks_check_state(t, count, streams))) return rc;
    cvo_batch bo = t->odo, bk = t->key;
    if ((rc = batch_settle(bo)) || (rc = batch_settle(bk))) return rc;
    std::vector<std::shared_ptr<Cloud>> in;
    if ((rc = clouds_ingest(bo, t->pool, count, clouds, cloud_stream, in))) return rc;     // (the step's one host wait; fails before any stream changes)
    std::vector<int> npts(count);
    for (int k = 0; k < count; ++k) npts[k] = clouds[k].n;
    return tracks_step_run(t, count, streams, npts.data(), &in, nullptr, hip_stream);
}
// ---- the next step's frames staged ahead: generated on the stage's own stream while the current step's launches run
int cvo_tracks_stage_async(cvo_tracks t, int count, const int* streams, const unsigned char* const* bgr8, const unsigned short* const* depth16, int width, int height,
                           const cvo_camera* cams, const int* cam_index) {
    const ImageSrc src = ImageSrc::host(bgr8, depth16);
    int rc = tracks_check_images(t, count, streams, src, width, height, cams, cam_index); if (rc) return rc;   // (an earlier stage survives a refused call)
    return stage_begin(t->odo, count, streams, src, width, height, cams, cam_index);
}
int cvo_tracks_stage_device_async(cvo_tracks t, int count, const int* streams, const cvo_device_image* images, int width, int height,
                                  const cvo_camera* cams, const int* cam_index, void* image_stream) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    int rc = check_device_images(t->odo->eng.device, count, images, width, height); if (rc) return rc;
    const ImageSrc src = ImageSrc::device(images, image_stream);
    if ((rc = tracks_check_images(t, count, streams, src, width, height, cams, cam_index))) return rc;
    return stage_begin(t->odo, count, streams, src, width, height, cams, cam_index);
}
int cvo_tracks_step_staged_async(cvo_tracks t, void* hip_stream) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    FrameStage& F = t->odo->stage;
    if (!F.pending) return fail(CVO_ERR_INVALID, "nothing staged (cvo_tracks_stage_async)");
    Lap lap(StepLaps::CONSUME);
    const int count = (int)F.list.size();
    int rc = tracks_check_state(t, count, F.list.data()); if (rc) return rc;   // (the stage is kept: commit, then call again)
    cvo_batch bo = t->odo, bk = t->key;
    if ((rc = batch_settle(bo)) || (rc = batch_settle(bk))) return rc;
    if ((rc = stage_take(bo))) return rc;                            // (fails before any stream changes; the stage is dropped)
    const std::vector<int> list = F.list, points = F.points;
    const std::vector<std::shared_ptr<Cloud>> clouds = F.clouds;
    stage_taken(bo);
    return tracks_step_run(t, count, list.data(), points.data(), &clouds, nullptr, hip_stream);
}
int cvo_tracks_staged_count(cvo_tracks t, int* images, long long* taken) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    return stage_count(t->odo, images, taken);
}
int cvo_tracks_done(cvo_tracks t, int* done) {
    if (!t || !done) return fail(CVO_ERR_INVALID, "null argument");
    *done = 1;
    if (!t->in_flight || t->n_odo == 0) return CVO_OK;
    return cvo_batch_done(t->n_key > 0 && t->key->eng.launched ? t->key : t->odo, done);
}
int cvo_tracks_wait(cvo_tracks t, cvo_track_step* out, int count) {
    if (!t) return fail(CVO_ERR_INVALID, "null tracks");
    if (!t->in_flight) return fail(CVO_ERR_INVALID, "no step to wait for");
    const int n = (int)t->list.size();
    if (out && count != n) return fail(CVO_ERR_INVALID, "one result per stream of the step");
    cvo_batch bo = t->odo, bk = t->key;
    int rc;
    Lap lap(StepLaps::WAIT);
    if (t->n_odo > 0 && (rc = batch_settle(bo))) return rc;          // (the odometry objects take their results in, as after cvo_batch_wait)
    if (t->n_key > 0 && (rc = bk->eng.wait())) return rc;
    const PairState* ro = bo->eng.results(); const PairState* rk = bk->eng.results();
    std::vector<unsigned char> want_o(std::max(t->n_odo, 1), 0), want_k(std::max(t->n_key, 1), 0);
    for (int k = 0; k < n; ++k) {
        if (t->odo_pos[k] >= 0) want_o[t->odo_pos[k]] = ro[t->odo_pos[k]].status == CVO_OK;
        if (t->key_pos[k] >= 0) want_k[t->key_pos[k]] = ro[t->odo_pos[k]].status == CVO_OK && rk[t->key_pos[k]].status == CVO_OK;
    }
    std::vector<cvo_track_scores> so(std::max(t->n_odo, 1)), sk(std::max(t->n_key, 1));
    std::memset(so.data(), 0, sizeof(cvo_track_scores) * so.size()); std::memset(sk.data(), 0, sizeof(cvo_track_scores) * sk.size());
    if (t->n_odo > 0 && (rc = tracks_scores(bo, t->n_odo, want_o, so))) return rc;
    if (t->n_key > 0 && (rc = tracks_scores(bk, t->n_key, want_k, sk))) return rc;
    const TrackLinkOut* lo = static_cast<const TrackLinkOut*>(t->h_link_out.p);
    t->odo_ok.assign(n, 0); t->key_ok.assign(n, 0);
    for (int k = 0; k < n; ++k) {
        if (t->odo_pos[k] >= 0) t->odo_ok[k] = want_o[t->odo_pos[k]];
        if (t->key_pos[k] >= 0) t->key_ok[k] = want_k[t->key_pos[k]];
    }
    for (int k = 0; k < n; ++k) {
        const int s = t->list[k];
        TrackStream& S = t->st[s]; KeyObject& K = S.key;
        cvo_track_step step; std::memset(&step, 0, sizeof(step));
        step.phase = t->phase[k]; step.points = t->points[k];
        step.odometry.status = step.keyframe.status = CVO_ERR_NOT_INITIALIZED;
        if (t->odo_pos[k] >= 0) {
            const PairState& r = ro[t->odo_pos[k]];
            pair_result_from(r, step.odometry); step.odometry_scores = so[t->odo_pos[k]];
            const bool odo_ok = r.status == CVO_OK;
            if (!odo_ok) {                                           // a failed alignment leaves the object as it was: report what it carries
                const StreamSlot& O = bo->streams[s];
                std::memcpy(step.odometry.R, O.R, sizeof(O.R)); std::memcpy(step.odometry.T, O.T, sizeof(O.T));
                std::memcpy(step.odometry.transform, O.transform.m, sizeof(O.transform.m));
                step.odometry.ell = O.ell; step.odometry.iter = O.iter;
            }
            if (t->phase[k] == 1 && odo_ok) {                        // local_tracker.cpp:330-333: first_frame = false; reset_transform(t_odometry)
                K.first_frame = false; std::memcpy(K.transform.m, r.transform, sizeof(K.transform.m));
            }
            if (t->phase[k] == 2 && !odo_ok) bk->moving[s] = t->moving_before[k];   // the keyframe object does not see this frame
            if (t->phase[k] == 2 && odo_ok) {
                const int i = t->key_pos[k];
                const PairState& q = rk[i];
                std::memcpy(K.R, lo[i].R, sizeof(K.R)); std::memcpy(K.T, lo[i].T, sizeof(K.T));   // reset_initial, local_tracker.cpp:407
                std::memcpy(step.initial_guess, lo[i].init_inverse, sizeof(step.initial_guess));
                pair_result_from(q, step.keyframe); step.keyframe_scores = sk[i];
                if (q.status == CVO_OK) {                            // what align() leaves behind (do_align)
                    std::memcpy(K.R, q.R, sizeof(K.R)); std::memcpy(K.T, q.T, sizeof(K.T));
                    K.ell = q.ell; K.iter = q.iter; K.A_nonzero = q.A_nonzero;
                    Aff prev; std::memcpy(prev.m, q.prev_transform, sizeof(prev.m));
                    K.prev_transform = prev; K.accum_transform = aff_mul(K.accum_transform, prev);
                    std::memcpy(K.transform.m, q.transform, sizeof(K.transform.m));
                } else {                                             // R, T stay as reset_initial set them, everything else as it was
                    std::memcpy(step.keyframe.R, K.R, sizeof(K.R)); std::memcpy(step.keyframe.T, K.T, sizeof(K.T));
                    std::memcpy(step.keyframe.transform, K.transform.m, sizeof(K.transform.m));
                    step.keyframe.ell = K.ell; step.keyframe.iter = K.iter; step.keyframe.A_nonzero = K.A_nonzero;
                }
                S.commit_pending = true;
                std::memcpy(S.t_odometry.m, r.transform, sizeof(S.t_odometry.m));
            }
        }
        if (out) out[k] = step;
    }
    t->moving_before.clear();
    t->in_flight = false;
    t->support_valid = true;
    return stage_place(bo, false);                                   // (frames staged while the step ran: placed now if their generator has finished too)
}
int cvo_tracks_commit(cvo_tracks t, int count, const int* streams, const int* accept) {
    int rc = tracks_check_list(t, count, streams); if (rc) return rc;
    if (!accept) return fail(CVO_ERR_INVALID, "null argument");
    if (t->in_flight) return fail(CVO_ERR_INVALID, "a step is in flight (cvo_tracks_wait first)");
    Lap lap(StepLaps::COMMIT);
    for (int k = 0; k < count; ++k)
        if (!t->st[streams[k]].commit_pending) return fail(CVO_ERR_INVALID, "stream " + std::to_string(streams[k]) + " expects no decision");
    t->support_valid = false;                                        // (the keyframe objects' clouds move on below)
    for (int k = 0; k < count; ++k) {
        const int s = streams[k];
        TrackStream& S = t->st[s]; KeyObject& K = S.key;
        std::shared_ptr<Cloud>& fixed = t->key->fixed[s]; std::shared_ptr<Cloud>& moving = t->key->moving[s];
        if (accept[k]) { K.previous = std::move(moving); K.pre_pc_init = true; }                        // update_previous_pcd, cvo.cpp:584-589
        else {                                                                                          // reset_keyframe(t_odometry), cvo.cpp:591-604
            if (!K.pre_pc_init) fixed = std::move(moving);
            else { fixed = std::move(K.previous); K.previous = std::move(moving); K.pre_pc_init = true; }
            K.transform = S.t_odometry;
        }
        moving.reset();
        S.commit_pending = false;
    }
    return CVO_OK;
}
namespace {
const Cloud* tracks_cloud(cvo_tracks_s* t, int s, int object, int slot) {
    cvo_batch b = object == 0 ? t->odo : t->key;
    if (slot == CVO_SLOT_FIXED) return b->fixed[s].get();
    if (slot == CVO_SLOT_MOVING) return b->moving[s].get();
    return object == 1 ? t->st[s].key.previous.get() : nullptr;
}
bool tracks_slot_ok(cvo_tracks_s* t, int s, int object, int slot) {
    return t && s >= 0 && s < t->max_streams && (object == 0 || object == 1) && (slot == CVO_SLOT_FIXED || slot == CVO_SLOT_MOVING || slot == CVO_SLOT_PREVIOUS);
}
}  // namespace
int cvo_tracks_get_cloud(cvo_tracks t, int s, int object, int slot, float* xyz, float* feat, int cap, int* n) {
    if (!n || !tracks_slot_ok(t, s, object, slot)) return fail(CVO_ERR_INVALID, "bad argument");
    return download_cloud(t->odo->eng, tracks_cloud(t, s, object, slot), xyz, feat, cap, n);
}
int cvo_tracks_get_selected_points(cvo_tracks t, int s, int object, int slot, unsigned short* px, int cap, int* n) {
    if (!n || !tracks_slot_ok(t, s, object, slot)) return fail(CVO_ERR_INVALID, "bad argument");
    return download_selected_points(t->odo->eng, tracks_cloud(t, s, object, slot), px, cap, n);
}
int cvo_tracks_get_state(cvo_tracks t, int s, int object, float R[9], float T[3], float* ell, float transform[12]) {
    if (!t || s < 0 || s >= t->max_streams || (object != 0 && object != 1)) return fail(CVO_ERR_INVALID, "bad argument");
    if (t->in_flight) return fail(CVO_ERR_INVALID, "a step is in flight (cvo_tracks_wait first)");
    const StreamSlot& O = t->odo->streams[s]; const KeyObject& K = t->st[s].key;
    if (R) std::memcpy(R, object == 0 ? O.R : K.R, sizeof(float) * 9);
    if (T) std::memcpy(T, object == 0 ? O.T : K.T, sizeof(float) * 3);
    if (ell) *ell = object == 0 ? O.ell : K.ell;
    if (transform) std::memcpy(transform, object == 0 ? O.transform.m : K.transform.m, sizeof(float) * 12);
    return CVO_OK;
}
namespace {
// what the point-support and point-matches calls of a tracker check alike: the listed streams' `object` aligned in the step waited for last
int tracks_aligned_slots(cvo_tracks_s* t, int object, int count, const int* streams, const void* dst, const std::string& who, std::vector<int>& slots) {
    int rc = tracks_check_list(t, count, streams); if (rc) return rc;
    if (!dst) return fail(CVO_ERR_INVALID, "null argument");
    if (object != 0 && object != 1) return fail(CVO_ERR_INVALID, "object must be 0 (odometry) or 1 (keyframe)");
    if (t->in_flight || !t->support_valid) return fail(CVO_ERR_INVALID, who + ": between cvo_tracks_wait of a step and the next cvo_tracks_commit or step only");
    slots.resize(count);
    for (int k = 0; k < count; ++k) {
        const int s = streams[k];
        int at = -1;
        for (size_t q = 0; q < t->list.size(); ++q) if (t->list[q] == s) at = (int)q;
        if (at < 0) return fail(CVO_ERR_INVALID, who + ": stream " + std::to_string(s) + " was not listed in the step");
        if (!(object == 0 ? t->odo_ok[at] : t->key_ok[at])) return fail(CVO_ERR_INVALID, who + ": that object of stream " + std::to_string(s) + " did not align in the step");
        slots[k] = s;                                                // (a stream's slot in both batches, and its device state's index)
    }
    return CVO_OK;
}
extern "C++" {
template <class Dst>
int tracks_sides(cvo_tracks_s* t, int object, int count, const int* streams, const Dst* dst, bool on_device, void* out_stream, const std::string& what) {
    std::vector<int> slots;
    int rc = tracks_aligned_slots(t, object, count, streams, dst, what, slots); if (rc) return rc;
    return batch_sides_run(object == 0 ? t->odo : t->key, slots, dst, on_device, out_stream, what);
}
}  // extern "C++"
}  // namespace
// ---- pose hypotheses (include/cvo_hip.h, "pose hypotheses"; cvo_hypothesis_kernels.hip)
namespace {
// what every hypothesis call checks about k, ell and the transforms before anything else happens
int hyp_check_args(int k, const float* trans, size_t n_trans, float ell) {
    if (!trans) return fail(CVO_ERR_INVALID, "hypotheses: null transform array");
    if (k < 1 || k > CVO_MAX_HYPOTHESES) return fail(CVO_ERR_INVALID, "hypotheses: k must be 1 .. CVO_MAX_HYPOTHESES");
    if (!std::isfinite(ell) || !(ell > 0.f)) return fail(CVO_ERR_INVALID, "hypotheses: ell must be finite and positive");
    for (size_t i = 0; i < 12 * n_trans; ++i) if (!std::isfinite(trans[i])) return fail(CVO_ERR_INVALID, "hypotheses: non-finite entry in transform " + std::to_string(i / 12));
    return CVO_OK;
}
// the listed slots of a batch call as requests; every argument error is found here, before anything is queued or changed
int batch_hyp_requests(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell, std::vector<int>& slots, std::vector<Engine::HypReq>& rq) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    if (count < 1 || count > b->max_pairs) return fail(CVO_ERR_INVALID, "hypotheses: bad pair count");
    int rc = hyp_check_args(k, trans, (size_t)count * (size_t)std::max(k, 0), ell); if (rc) return rc;
    std::vector<unsigned char> seen(b->max_pairs, 0);
    slots.resize(count); rq.resize(count);
    for (int i = 0; i < count; ++i) {
        const int p = pairs ? pairs[i] : i;
        if (p < 0 || p >= b->max_pairs) return fail(CVO_ERR_INVALID, "hypotheses: slot " + std::to_string(p) + " out of range");
        if (seen[p]++) return fail(CVO_ERR_INVALID, "hypotheses: slot " + std::to_string(p) + " listed twice");
        if (b->streams[p].on) return fail(CVO_ERR_INVALID, "hypotheses: slot " + std::to_string(p) + " is a stream slot (it carries its own state)");
        slots[i] = p;
    }
    for (int i = 0; i < count; ++i) {
        const Cloud* fx = b->fixed[slots[i]].get(); const Cloud* mv = b->moving[slots[i]].get();
        if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "hypotheses: empty cloud in slot " + std::to_string(slots[i]));
        rq[i] = Engine::HypReq{mv, fx, slots[i], &b->init_states[slots[i]]};
    }
    return CVO_OK;
}
}  // namespace

int cvo_score_hypotheses(cvo_handle h, int slot_a, int slot_b, int k, const float* trans, float ell, cvo_inn_p* scores, int* best) {
    if (!h || !scores) return fail(CVO_ERR_INVALID, "null argument");
    int rc = hyp_check_args(k, trans, (size_t)std::max(k, 0), ell); if (rc) return rc;
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "hypotheses: empty cloud slot");
    const Engine::HypReq rq[1] = {{a, b, -1, nullptr}};
    if ((rc = h->eng.hyp_enqueue(rq, 1, k, trans, ell, h->eng.stream, false))) return rc;
    return h->eng.hyp_collect(scores, best);
}
int cvo_batch_score_hypotheses(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell, cvo_inn_p* scores, int* best) {
    if (!scores) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<int> slots; std::vector<Engine::HypReq> rq;
    int rc = batch_hyp_requests(b, count, pairs, k, trans, ell, slots, rq); if (rc) return rc;
    if ((rc = batch_settle(b))) return rc;
    if ((rc = b->eng.hyp_enqueue(rq.data(), count, k, trans, ell, b->eng.stream, false))) return rc;
    return b->eng.hyp_collect(scores, best);
}
int cvo_batch_seed_hypotheses_async(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell) {
    std::vector<int> slots; std::vector<Engine::HypReq> rq;
    int rc = batch_hyp_requests(b, count, pairs, k, trans, ell, slots, rq); if (rc) return rc;
    if ((rc = batch_settle(b))) return rc;
    if ((rc = b->eng.hyp_enqueue(rq.data(), count, k, trans, ell, b->eng.stream, true))) return rc;
    for (int p : slots) b->dirty[p] = 0;                             // the next launch that lists them starts from what the select step wrote (Engine::launch: upload_each == 0)
    return CVO_OK;
}
int cvo_batch_hypothesis_results(cvo_batch b, int count, cvo_inn_p* scores, int* best) {
    if (!b) return fail(CVO_ERR_INVALID, "null batch");
    Engine& E = b->eng;
    const bool pending = E.hyp_call.queued && E.hyp_seed;
    if (count < 1 || count > (pending ? E.hyp_n : E.seed_n)) return fail(CVO_ERR_INVALID, "hypothesis results: no seeding call of that many pairs");
    HIP_TRY(hipSetDevice(E.device));
    int rc = E.hyp_keep(); if (rc) return rc;                        // (waits for the seeding call's two kernels alone: their own event)
    if (scores) std::memcpy(scores, E.seed_scores.data(), sizeof(cvo_inn_p) * (size_t)count * E.seed_k);
    if (best) std::memcpy(best, E.seed_best.data(), sizeof(int) * (size_t)count);
    return CVO_OK;
}

// ---- pose models (include/cvo_hip.h, "pose models"; cvo_pose_model_kernels.hip)
int cvo_pose_models(cvo_handle h, int slot_a, int slot_b, int k, const float* trans, float ell, cvo_pose_model* out) {
    if (!h || !out) return fail(CVO_ERR_INVALID, "null argument");
    int rc = hyp_check_args(k, trans, (size_t)std::max(k, 0), ell); if (rc) return rc;
    Cloud* a = slot_cloud(h, slot_a); Cloud* b = slot_cloud(h, slot_b);
    if (!a || !b || a->n <= 0 || b->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "pose models: empty cloud slot");
    const Engine::PoseModelReq rq[1] = {{a, b, -1}};
    if ((rc = h->eng.pm_enqueue(rq, 1, k, trans, ell, h->eng.stream))) return rc;
    return h->eng.pm_collect(out);
}
int cvo_batch_pose_models(cvo_batch b, int count, const int* pairs, int k, const float* trans, float ell, cvo_pose_model* out) {
    if (!out) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<int> slots; std::vector<Engine::HypReq> hq;
    int rc = batch_hyp_requests(b, count, pairs, k, trans, ell, slots, hq); if (rc) return rc;   // the rules and errors of cvo_batch_score_hypotheses
    std::vector<Engine::PoseModelReq> rq(count);
    for (int i = 0; i < count; ++i) rq[i] = Engine::PoseModelReq{hq[i].a, hq[i].b, -1};
    if ((rc = batch_settle(b))) return rc;
    if ((rc = b->eng.pm_enqueue(rq.data(), count, k, trans, ell, b->eng.stream))) return rc;
    return b->eng.pm_collect(out);
}
int cvo_batch_result_models(cvo_batch b, int count, const int* pairs, cvo_pose_model* out) {
    if (!b || !out) return fail(CVO_ERR_INVALID, "null argument");
    std::vector<Engine::PoseModelReq> rq;
    int rc = last_launch_pairs(b, count, pairs, "result models", [&](int k, int p) {
        if (k == 0) rq.reserve(count);
        const Cloud* fx = b->fixed[p].get(); const Cloud* mv = b->moving[p].get();
        if (!fx || !mv || fx->n <= 0 || mv->n <= 0) return fail(CVO_ERR_EMPTY_CLOUD, "result models: empty cloud in the batch");
        rq.push_back(Engine::PoseModelReq{mv, fx, p});               // transform and ell: the pair's device-resident state, as cvo_batch_point_support reads it
        return (int)CVO_OK;
    });
    if (rc) return rc;
    if ((rc = b->eng.pm_enqueue(rq.data(), count, 1, nullptr, 0.f, b->eng.last_stream))) return rc;   // behind the align launch on its stream
    return b->eng.pm_collect(out);
}

int cvo_tracks_point_support(cvo_tracks t, int object, int count, const int* streams, const cvo_point_support_dst* dst) {
    return tracks_sides(t, object, count, streams, dst, false, nullptr, "point support");
}
int cvo_tracks_point_support_device(cvo_tracks t, int object, int count, const int* streams, const cvo_point_support_dst* dst, void* out_stream) {
    return tracks_sides(t, object, count, streams, dst, true, out_stream, "point support");
}
int cvo_tracks_point_matches(cvo_tracks t, int object, int count, const int* streams, const cvo_point_matches_dst* dst) {
    return tracks_sides(t, object, count, streams, dst, false, nullptr, "point matches");
}
int cvo_tracks_point_matches_device(cvo_tracks t, int object, int count, const int* streams, const cvo_point_matches_dst* dst, void* out_stream) {
    return tracks_sides(t, object, count, streams, dst, true, out_stream, "point matches");
}

// ---------------------------------------------------------------- multi-GPU: RCCL all-gather of the result records
}  // extern "C"

namespace {
// RCCL is bound at run time (dlopen) so that single-GPU users of the library do not need it at load time.
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, /* ncclUniqueId by value: 128 bytes */ struct Id128, int) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*CommUserRank)(void*, int*) = nullptr;
};
struct Id128 { char b[CVO_COMM_ID_BYTES]; };
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.lib) return CVO_OK;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (h) break; }
    if (!h) return fail(CVO_ERR_HIP, std::string("RCCL not found (librccl.so.1): ") + (dlerror() ? dlerror() : ""));
#define CVO_RCCL_SYM(field, sym) do { *reinterpret_cast<void**>(&g_rccl.field) = dlsym(h, sym); if (!g_rccl.field) return fail(CVO_ERR_HIP, std::string("RCCL symbol missing: ") + sym); } while (0)
    CVO_RCCL_SYM(GetUniqueId, "ncclGetUniqueId"); CVO_RCCL_SYM(CommInitRank, "ncclCommInitRank"); CVO_RCCL_SYM(CommInitAll, "ncclCommInitAll");
    CVO_RCCL_SYM(CommDestroy, "ncclCommDestroy"); CVO_RCCL_SYM(AllGather, "ncclAllGather"); CVO_RCCL_SYM(GroupStart, "ncclGroupStart");
    CVO_RCCL_SYM(GroupEnd, "ncclGroupEnd"); CVO_RCCL_SYM(GetErrorString, "ncclGetErrorString");
    CVO_RCCL_SYM(CommCount, "ncclCommCount"); CVO_RCCL_SYM(CommUserRank, "ncclCommUserRank");
#undef CVO_RCCL_SYM
    g_rccl.lib = h;
    return CVO_OK;
}
#define RCCL_TRY(expr) do { int r__ = (expr); if (r__ != 0) return fail(CVO_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r__)); } while (0)
constexpr int RCCL_FLOAT = 7;     // ncclFloat32 (rccl.h)
}  // namespace

// `send`: a block of records that all carry CVO_ERR_RANK_FAILED, made when the communicator is: what this rank contributes to a gather whose own block
// could not be prepared (bad arguments, a buffer that would not grow, a fill kernel that would not launch) -- so that the rank still enters the collective.
// own_stream (cvo_comm_set_gather_stream; CVO_HIP_GATHER_STREAM=1 when the communicator is made): every gather of this communicator runs on ONE stream of the
// communicator's own, behind an event of the align launch it follows, and the launch's stream continues behind the gather's event -- the fallback for a RCCL that
// does not take collectives of one communicator from several streams at once.
struct cvo_comm_s { void* comm = nullptr; int n_ranks = 1, rank = 0, device = 0; DevBuf send; int fallback_records = 0;
                    bool own_stream = false; hipStream_t gstream = nullptr; hipEvent_t ev_in = nullptr, ev_out = nullptr; };

struct cvo_multi_s {
    int n_devices = 0, max_pairs = 0, last_n = 0;
    std::vector<int> devices;
    std::vector<cvo_batch> batches;
    std::vector<cvo_comm> comms;
    std::vector<DevBuf> recv;
};

namespace {
constexpr int COMM_FALLBACK_RECORDS = 1024;        // 64 KB; a gather of larger blocks grows it when it is first needed
// (re)make the communicator's block of failure records; the device is current.  Not fatal when it cannot be made: the communicator works without it,
// a failed prepare then returns without entering the collective (and says so).
int comm_fallback_block(cvo_comm_s* c, int records) {
    if (records <= c->fallback_records) return CVO_OK;
    c->fallback_records = 0;
    int rc = c->send.ensure(sizeof(float) * CVO_RESULT_FLOATS * (size_t)records); if (rc) return rc;
    hipError_t e = cvohip::launch_fill_records(static_cast<float*>(c->send.p), 0, records, CVO_ERR_RANK_FAILED, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(CVO_ERR_HIP, std::string("failure-record block: ") + hipGetErrorString(e));
    c->fallback_records = records;
    return CVO_OK;
}
}  // namespace

extern "C" {

int cvo_shard_range(int n_pairs_total, int rank, int n_ranks, int* first, int* count) {
    if (n_pairs_total < 0 || n_ranks <= 0 || rank < 0 || rank >= n_ranks || !first || !count) return fail(CVO_ERR_INVALID, "bad shard arguments");
    const int base = n_pairs_total / n_ranks, rem = n_pairs_total % n_ranks;      // block sizes differ by at most one
    *first = rank * base + std::min(rank, rem); *count = base + (rank < rem ? 1 : 0);
    return CVO_OK;
}
int cvo_comm_unique_id(char id[CVO_COMM_ID_BYTES]) {
    if (!id) return fail(CVO_ERR_INVALID, "null id");
    int rc = rccl_load(); if (rc) return rc;
    RCCL_TRY(g_rccl.GetUniqueId(id));
    return CVO_OK;
}
int cvo_comm_create(const char id[CVO_COMM_ID_BYTES], int n_ranks, int rank, int device, cvo_comm* out) {
    if (!id || !out || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(CVO_ERR_INVALID, "bad communicator arguments");
    int rc = check_device(device, nullptr); if (rc) return rc;
    rc = rccl_load(); if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    Id128 uid; std::memcpy(uid.b, id, CVO_COMM_ID_BYTES);
    void* comm = nullptr;
    RCCL_TRY(g_rccl.CommInitRank(&comm, n_ranks, uid, rank));
    cvo_comm_s* c = new cvo_comm_s(); c->comm = comm; c->n_ranks = n_ranks; c->rank = rank; c->device = device;
    if (const char* e = std::getenv("CVO_HIP_GATHER_STREAM")) c->own_stream = std::atoi(e) != 0;
    (void)comm_fallback_block(c, COMM_FALLBACK_RECORDS);
    *out = c;
    return CVO_OK;
}
int cvo_comm_create_all(const int* devices, int n_devices, cvo_comm* out) {
    if (!devices || !out || n_devices <= 0) return fail(CVO_ERR_INVALID, "bad communicator arguments");
    for (int i = 0; i < n_devices; ++i) { int rc = check_device(devices[i], nullptr); if (rc) return rc; }
    int rc = rccl_load(); if (rc) return rc;
    std::vector<void*> comms(n_devices, nullptr);
    RCCL_TRY(g_rccl.CommInitAll(comms.data(), n_devices, devices));
    for (int i = 0; i < n_devices; ++i) {
        cvo_comm_s* c = new cvo_comm_s(); c->comm = comms[i]; c->n_ranks = n_devices; c->rank = i; c->device = devices[i];
        if (const char* e = std::getenv("CVO_HIP_GATHER_STREAM")) c->own_stream = std::atoi(e) != 0;
        if (hipSetDevice(devices[i]) == hipSuccess) (void)comm_fallback_block(c, COMM_FALLBACK_RECORDS);
        out[i] = c;
    }
    return CVO_OK;
}
// what the communicator itself says (ncclCommCount / ncclCommUserRank), not what it was asked for
int cvo_comm_info(cvo_comm c, int* n_ranks, int* rank) {
    if (!c || !c->comm) return fail(CVO_ERR_INVALID, "null communicator");
    int n = 0, r = 0;
    RCCL_TRY(g_rccl.CommCount(c->comm, &n)); RCCL_TRY(g_rccl.CommUserRank(c->comm, &r));
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    return CVO_OK;
}
int cvo_comm_set_gather_stream(cvo_comm c, int on) {
    if (!c) return fail(CVO_ERR_INVALID, "null communicator");
    c->own_stream = on != 0; return CVO_OK;
}
// where the RCCL this process bound lives on disk (dladdr of ncclAllGather): a torch process resolves librccl.so.1 to torch's bundled copy, a plain C++ caller to /opt/rocm's
int cvo_comm_library_path(char* out, int cap) {
    if (!out || cap <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    out[0] = 0;
    int rc = rccl_load(); if (rc) return rc;
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(g_rccl.AllGather), &info) && info.dli_fname) { std::strncpy(out, info.dli_fname, (size_t)cap - 1); out[cap - 1] = 0; }
    return CVO_OK;
}
int cvo_comm_destroy(cvo_comm c) {
    if (!c) return fail(CVO_ERR_INVALID, "null communicator");
    (void)hipSetDevice(c->device);
    if (c->gstream) { (void)hipStreamSynchronize(c->gstream); (void)hipStreamDestroy(c->gstream); (void)hipEventDestroy(c->ev_in); (void)hipEventDestroy(c->ev_out); }
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    c->send.release();
    delete c;
    return CVO_OK;
}
namespace {
// Everything of a gather that can fail happens here, BEFORE the collective is entered: argument checks, the record block (growth,
// padding / status records).  The all-gather itself is posted by gather_post and reads the block in stream order.  When the preparation
// fails, gather_fallback_plan points the plan at the communicator's block of CVO_ERR_RANK_FAILED records instead: the rank still enters the
// collective (its peers read the failure in the gathered table instead of waiting for the rank forever) and the call returns the error.
struct GatherPlan { hipStream_t s = nullptr; float* send = nullptr; };
int gather_prepare(cvo_batch b, cvo_comm c, int n_valid, int n_block, int launch_status, void* recv_device, GatherPlan& plan) {
    if (!b || !c || !recv_device) return fail(CVO_ERR_INVALID, "bad gather arguments");
    if (c->device != b->eng.device) return fail(CVO_ERR_INVALID, "communicator and batch live on different devices");
    return b->eng.padded_records(n_valid, n_block, launch_status, b->last_n, &plan.s, &plan.send);
}
bool gather_fallback_plan(cvo_batch b, cvo_comm c, int n_block, void* recv_device, GatherPlan& plan) {
    if (!c || !c->comm || !recv_device || n_block <= 0) return false;                 // nothing to enter the collective with
    if (hipSetDevice(c->device) != hipSuccess) return false;
    if (n_block > c->fallback_records && comm_fallback_block(c, n_block) != CVO_OK) return false;
    // behind the rank's launch when there is one on this device (the peers' gathers of this step are ordered behind theirs), else the null stream
    plan.s = (b && b->eng.device == c->device) ? (b->eng.launched ? b->eng.last_stream : b->eng.stream) : nullptr;
    plan.send = static_cast<float*>(c->send.p);
    return true;
}
int gather_post(cvo_comm c, int n_block, void* recv_device, const GatherPlan& plan) {
    if (c->own_stream) {
        // launch stream -> event -> the communicator's stream: all-gather -> event -> the launch stream waits for it: whoever waits for the launch's stream
        // (cvo_batch_wait) still finds every rank's records in place, and the collectives of this communicator are posted to one stream, in call order
        if (!c->gstream) { HIP_TRY(hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking)); HIP_TRY(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming)); }
        HIP_TRY(hipEventRecord(c->ev_in, plan.s));
        HIP_TRY(hipStreamWaitEvent(c->gstream, c->ev_in, 0));
        RCCL_TRY(g_rccl.AllGather(plan.send, recv_device, (size_t)n_block * CVO_RESULT_FLOATS, RCCL_FLOAT, c->comm, c->gstream));
        HIP_TRY(hipEventRecord(c->ev_out, c->gstream));
        HIP_TRY(hipStreamWaitEvent(plan.s, c->ev_out, 0));
        return CVO_OK;
    }
    RCCL_TRY(g_rccl.AllGather(plan.send, recv_device, (size_t)n_block * CVO_RESULT_FLOATS, RCCL_FLOAT, c->comm, plan.s));
    return CVO_OK;
}
}  // namespace
int cvo_shard_block(int n_pairs_total, int n_ranks) { return (n_pairs_total < 0 || n_ranks <= 0) ? 0 : (n_pairs_total + n_ranks - 1) / n_ranks; }
int cvo_batch_padded_records(cvo_batch b, int n_valid, int n_block, int launch_status, const void** send_device) {
    if (!b || !send_device) return fail(CVO_ERR_INVALID, "null argument");
    hipStream_t s; float* send;
    int rc = b->eng.padded_records(n_valid, n_block, launch_status, b->last_n, &s, &send); if (rc) return rc;
    *send_device = send;
    return CVO_OK;
}
int cvo_batch_gather_results_padded(cvo_batch b, cvo_comm c, int n_valid, int n_block, int launch_status, void* recv_device) {
    int rc = rccl_load(); if (rc) return rc;
    GatherPlan plan;
    rc = gather_prepare(b, c, n_valid, n_block, launch_status, recv_device, plan);
    if (rc) {                                                       // the rank enters the collective all the same, with failure records
        const std::string msg = g_err;
        if (gather_fallback_plan(b, c, n_block, recv_device, plan) && gather_post(c, n_block, recv_device, plan) == CVO_OK)
            return fail(rc, msg + " (collective entered with CVO_ERR_RANK_FAILED records)");
        return fail(rc, msg + " (collective NOT entered)");
    }
    return gather_post(c, n_block, recv_device, plan);
}
int cvo_batch_gather_results(cvo_batch b, cvo_comm c, int n, void* recv_device) {
    return cvo_batch_gather_results_padded(b, c, n, n, CVO_OK, recv_device);
}
int cvo_gather_results_padded(cvo_batch* batches, cvo_comm* comms, int n_devices, const int* n_valid, int n_block, const int* launch_status, void* const* recv_device) {
    if (!batches || !comms || !recv_device || !n_valid || n_devices <= 0) return fail(CVO_ERR_INVALID, "bad gather arguments");
    int rc = rccl_load(); if (rc) return rc;
    std::vector<GatherPlan> plans(n_devices);
    int first_err = CVO_OK; std::string first_msg;
    for (int i = 0; i < n_devices; ++i) {                            // nothing can fail inside the RCCL group: a rank enqueued without its peers would wait for ever
        rc = gather_prepare(batches[i], comms[i], n_valid[i], n_block, launch_status ? launch_status[i] : CVO_OK, recv_device[i], plans[i]);
        if (rc) {                                                   // this device sends failure records; the error is reported after the collective is posted
            if (!first_err) { first_err = rc; first_msg = g_err + " (collective entered with CVO_ERR_RANK_FAILED records)"; }
            if (!gather_fallback_plan(batches[i], comms[i], n_block, recv_device[i], plans[i])) return fail(rc, first_msg = g_err + " (collective NOT entered)");
        }
    }
    RCCL_TRY(g_rccl.GroupStart());                                  // one process drives several ranks: their calls must be grouped
    for (int i = 0; i < n_devices; ++i) {
        const int r = gather_post(comms[i], n_block, recv_device[i], plans[i]);
        if (r && !first_err) { first_err = r; first_msg = g_err; }
    }
    const int ge = g_rccl.GroupEnd();
    if (first_err) return fail(first_err, first_msg);
    if (ge != 0) return fail(CVO_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(ge));
    return CVO_OK;
}
int cvo_gather_results(cvo_batch* batches, cvo_comm* comms, int n_devices, int n, void* const* recv_device) {
    if (n_devices <= 0) return fail(CVO_ERR_INVALID, "bad gather arguments");
    std::vector<int> nv(n_devices, n);
    return cvo_gather_results_padded(batches, comms, n_devices, nv.data(), n, nullptr, recv_device);
}
// rank-major gathered blocks (n_ranks x cvo_shard_block records) -> the n_pairs_total records in global pair order
int cvo_compact_records(const float* gathered, int n_pairs_total, int n_ranks, float* out, int* first_error) {
    if (!gathered || !out || n_pairs_total < 0 || n_ranks <= 0) return fail(CVO_ERR_INVALID, "bad argument");
    const int blk = cvo_shard_block(n_pairs_total, n_ranks);
    int err = CVO_OK;
    for (int r = 0; r < n_ranks; ++r) {
        int first = 0, count = 0; cvo_shard_range(n_pairs_total, r, n_ranks, &first, &count);
        const float* src = gathered + (size_t)r * blk * CVO_RESULT_FLOATS;
        for (int k = 0; k < count; ++k) {
            std::memcpy(out + (size_t)(first + k) * CVO_RESULT_FLOATS, src + (size_t)k * CVO_RESULT_FLOATS, sizeof(float) * CVO_RESULT_FLOATS);
            const int st = (int)src[(size_t)k * CVO_RESULT_FLOATS + 15];
            if (st != CVO_OK && err == CVO_OK) err = st;
        }
    }
    if (first_error) *first_error = err;
    return CVO_OK;
}

int cvo_multi_create(const cvo_params* p, const int* devices, int n_devices, int max_pairs_per_device, cvo_multi* out) {
    if (!devices || !out || n_devices <= 0 || max_pairs_per_device <= 0) return fail(CVO_ERR_INVALID, "bad multi arguments");
    std::unique_ptr<cvo_multi_s> m(new cvo_multi_s());
    m->n_devices = n_devices; m->max_pairs = max_pairs_per_device; m->devices.assign(devices, devices + n_devices);
    m->batches.assign(n_devices, nullptr); m->comms.assign(n_devices, nullptr); m->recv.resize(n_devices);
    int rc = cvo_comm_create_all(devices, n_devices, m->comms.data());
    for (int i = 0; i < n_devices && !rc; ++i) rc = cvo_batch_create(p, devices[i], max_pairs_per_device, &m->batches[i]);
    for (int i = 0; i < n_devices && !rc; ++i) {
        rc = (hipSetDevice(devices[i]) == hipSuccess) ? m->recv[i].ensure(sizeof(float) * (size_t)n_devices * max_pairs_per_device * CVO_RESULT_FLOATS)
                                                      : fail(CVO_ERR_HIP, "hipSetDevice failed");
    }
    if (rc) { const std::string msg = g_err; cvo_multi_destroy(m.release()); g_err = msg; return rc; }
    *out = m.release();
    return CVO_OK;
}
int cvo_multi_destroy(cvo_multi m) {
    if (!m) return fail(CVO_ERR_INVALID, "null multi");
    for (int i = 0; i < m->n_devices; ++i) {
        if (m->batches[i]) (void)cvo_batch_destroy(m->batches[i]);
        if (m->comms[i]) (void)cvo_comm_destroy(m->comms[i]);
        (void)hipSetDevice(m->devices[i]); m->recv[i].release();
    }
    delete m;
    return CVO_OK;
}
int cvo_multi_batch(cvo_multi m, int i, cvo_batch* out) {
    if (!m || !out || i < 0 || i >= m->n_devices) return fail(CVO_ERR_INVALID, "bad device index");
    *out = m->batches[i];
    return CVO_OK;
}
// n_pairs[i] pairs on device i (0 = none: the device only contributes padding).  Every device enters the gather whatever its launch
// returned: a launch that could not be made turns into status records, and the first error is reported after the collective is posted.
int cvo_multi_align_async_v(cvo_multi m, const int* n_pairs) {
    if (!m || !n_pairs) return fail(CVO_ERR_INVALID, "null argument");
    int n_block = 0;
    for (int i = 0; i < m->n_devices; ++i) {
        if (n_pairs[i] < 0 || n_pairs[i] > m->max_pairs) return fail(CVO_ERR_INVALID, "bad pair count");
        n_block = std::max(n_block, n_pairs[i]);
    }
    if (n_block <= 0) return fail(CVO_ERR_INVALID, "no pairs on any device");
    std::vector<int> st(m->n_devices, CVO_OK), nv(m->n_devices, 0);
    int first_err = CVO_OK; std::string first_msg;
    for (int i = 0; i < m->n_devices; ++i) {
        if (n_pairs[i] > 0) st[i] = cvo_batch_align_async(m->batches[i], n_pairs[i], nullptr);
        if (st[i] && !first_err) { first_err = st[i]; first_msg = g_err; }
        nv[i] = st[i] ? 0 : n_pairs[i];
    }
    std::vector<void*> recv(m->n_devices);
    for (int i = 0; i < m->n_devices; ++i) recv[i] = m->recv[i].p;
    int rc = cvo_gather_results_padded(m->batches.data(), m->comms.data(), m->n_devices, nv.data(), n_block, st.data(), recv.data()); if (rc) return rc;
    m->last_n = n_block;
    if (first_err) return fail(first_err, first_msg);
    return CVO_OK;
}
int cvo_multi_align_async(cvo_multi m, int n) {
    if (!m || n <= 0 || n > m->max_pairs) return fail(CVO_ERR_INVALID, "bad pair count");
    std::vector<int> nv(m->n_devices, n);
    return cvo_multi_align_async_v(m, nv.data());
}
int cvo_multi_wait(cvo_multi m, int from_device, float* records_out) {
    if (!m || from_device < 0 || from_device >= m->n_devices) return fail(CVO_ERR_INVALID, "bad argument");
    if (m->last_n <= 0) return fail(CVO_ERR_INVALID, "no launch to wait for");
    for (int i = 0; i < m->n_devices; ++i) {
        Engine& e = m->batches[i]->eng;
        if (e.launched) { int rc = cvo_batch_wait(m->batches[i], nullptr, 0); if (rc) return rc; }
        else { HIP_TRY(hipSetDevice(e.device)); HIP_TRY(hipStreamSynchronize(e.stream)); }   // the device only sent padding: its gather ran on the engine's own stream
    }
    if (records_out) {
        HIP_TRY(hipSetDevice(m->devices[from_device]));
        HIP_TRY(hipMemcpy(records_out, m->recv[from_device].p, sizeof(float) * (size_t)m->n_devices * m->last_n * CVO_RESULT_FLOATS, hipMemcpyDeviceToHost));
    }
    return CVO_OK;
}

}  // extern "C"
