// cvo_device.h -- device-side data structures shared by the HIP kernels and the
// host-side C-ABI implementation (cvo_capi.hip).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvohip {

// A cloud of n points in HBM is two planes of n float4: {x, y, z, f0} -- the reference's position
// (data_type.h:30) and the first channel of its 5-channel feature row (data_type.h:75), all that the
// transform, the cull and the geometric half of the kernel value touch -- then {f1, f2, f3, f4}.
// Consecutive lanes fetch consecutive 16-byte records of one plane.
constexpr int REC = 8;                   // floats per point over both planes
__host__ __device__ inline size_t lo_off(int i) { return (size_t)i * 4; }
__host__ __device__ inline size_t hi_off(int n, int i) { return ((size_t)n + (size_t)i) * 4; }
constexpr int MAX_ROWS_PER_WG = 4096;   // fixed-cloud rows one workgroup can own (LDS row-offset table)

struct DevParams {           // cvo.cpp:35-51
    float sigma, sp_thres, c, d, c_ell, c_sigma, min_step, eps, eps_2;
    int max_iter;
    float skin;              // candidate lists are built with radius (1+skin)*r and reused until the cloud has moved skin*r
    float skin_alpha;        // depth-proportional part of the list margin: a moving point may travel skin*r + skin_alpha*|y| (its distance from the camera when the lists were
                             // built) before the lists are stale -- a rotation moves far points most, and far rows have few neighbours (density falls with 1/z^2), so their
                             // wider lists cost little; row i's list radius is (r (1 + skin) + skin_alpha |x_i|) / (1 - skin_alpha).  0 = one margin for all rows
    int fuse_refine;         // the last candidate walk at an ell also makes the next ell's lists (cand_steady<REFINE>) instead of a filter pass of its own at the drop (CVO_HIP_FUSE_REFINE)
    float first_scale;       // the margins of a pair's first lists (built before any twist is known) are this many times skin / skin_alpha
    float alpha_gamma;       // skin_alpha applies at ell = 0.15 and falls with (ell / 0.15)^alpha_gamma (0 = the same at every ell)
    float predict;           // candidate lists are built around positions extrapolated along the previous iteration's twist, this fraction of every point's allowance ahead
                             // (0 = at the current positions); predict_steps caps the extrapolation in units of the last iteration's step
    float predict_steps;
    int overlap_stop_test;   // the next iteration's transform starts before the second stop test of this one (dist_se3) is done (phase_epilogue); 0 = behind it (CVO_HIP_OVERLAP_STOP)
    int nt_min;              // experiment (CVO_HIP_NT_MIN): lists of fewer entries than this are read with plain loads instead of non-temporal ones (0 = always non-temporal)
    int resort;              // rows re-sorted after a list refinement: 0 never, 1 when the cost model says it pays (default), 2 always (tests)
    int colocate;            // the workgroups of a pair on ONE XCD (blocks b, b + 8, ... share one): they read the same moving cloud and swap partial sums through
                             // L2 twice per iteration.  Takes a launch whose pair slots are a multiple of 8; 0 = consecutive blocks (four XCDs for G = 4)
    int adopt_kmax;          // adoption: a finished workgroup only offers its help to pairs with fewer iterations than this behind them (the heavy
                             // early iterations divide well between workgroups; the light late ones are bound by the iteration's fixed latency)
    int adopt_on;            // set per launch by the host, two bits.  ADOPT_ON_HELP: finished workgroups of this launch may help with its pairs that still run (one
                             // workgroup and one slot per pair).  ADOPT_ON_DEFERRED: the launch was queued behind launches of this library on every hardware queue,
                             // so it was not counted as submitted; its workgroups count themselves as deferred when they start (cvo_capi.hip, AdoptCounters)
    int adopt_inject;        // test knob (CVO_HIP_ADOPT_INJECT): 1 = a helper whose offer has been accepted leaves instead of confirming -- the owner must take the
                             // acceptance back and carry on with the members it has
    int adopt_dwell;         // adoption: a finished workgroup offers its help only when nothing has been queued on the device for this long (ticks of 10 ns; 0 = at once):
                             // a caller that resubmits as launches complete leaves the queue dry for a moment each time, and a helper that joins then holds its CU
                             // for the rest of the pair while the next launch's workgroups wait for one (CVO_HIP_ADOPT_DWELL_US)
};
constexpr int ADOPT_ON_HELP = 1, ADOPT_ON_DEFERRED = 2;   // DevParams::adopt_on

// per-pair state, read at kernel start and written back at the end (Q1, Q2)
struct PairState {
    float R[9];
    float T[3];
    float ell;
    float transform[12];      // in: cvo::transform before the call; out: final [R^T | -R^T T] (cvo.cpp:817)
    float prev_transform[12]; // out: transform of the last executed iteration (cvo.cpp:815)
    int iter;                 // value of k at the break (stale if max_iter is hit, Q4)
    int A_nonzero;            // nnz of the last iteration (Q5)
    int iterations_run;
    int status;
    int joined_at;            // iteration at which a finished workgroup of the launch joined this pair (adoption), 0 = none
    int adopt_retracted;      // acceptances the owner took back because the helper did not confirm in time (adoption)
    int rebuilds;             // dense culls executed
    int dense_fallbacks;      // rebuilds whose candidates did not fit the lists (dense per-row path taken)
    long long candidates_total;
    long long nonzeros_total; // nonzeros of A summed over the executed iterations (the reference's work: cvo.cpp:166-175 members, :282-306 terms)
    // wall time (100 MHz ticks) workgroup 0 of the pair spent per phase (slots as cvo_batch_last_phase_seconds documents them)
    unsigned long long clk_cycles, clk_ticks;   // shader-clock cycles and 100 MHz ticks workgroup 0 spent on the pair: cycles/ticks*100 MHz = clock
    unsigned long long tail_ticks[4];           // the score block in the kernel's tail (phase_tail_scores), 100 MHz ticks of workgroup 0: transform + list walk (inn_post, Hessian), the cull for inn_pre, its walk, all of it
    unsigned long long predict_mask;            // ... and the cull built its lists around extrapolated positions (DevParams::predict)
    unsigned long long cull_mask;               // bit min(k, 63) set: iteration k began with a dense cull (diagnostics: when do the lists go stale)
    unsigned long long clk_t0;                  // the device's 100 MHz counter when workgroup 0 took the pair up (one counter for the whole device: launches can be laid on one time axis)
    unsigned long long phase_ticks[10];
};

struct TraceRow {        // == cvo_trace_row (include/cvo_hip.h)
    float omega[3];
    float v[3];
    int nnz;
    int candidates;
    double B, C, D, E;
    float step;
    float ell;
    float dist;
    int pad_;
};

// arithmetic modes (include/cvo_hip.h: CVO_ARITH_*, the bits of the test oracle's ORC_VAR_*): run by the CVO_ARITH_MODES builds of the align kernel
constexpr int ARITH_F32_ROOTS = 2, ARITH_F32_LOGM = 4, ARITH_ROW_LAZY16 = 8, ARITH_ALL = ARITH_F32_ROOTS | ARITH_F32_LOGM | ARITH_ROW_LAZY16;

constexpr int TAIL_PRE = 1, TAIL_POST = 2, TAIL_FIXED = 4, TAIL_MOVING = 8, TAIL_HESSIAN = 16;   // PairDesc::score_out[23]

// exchange area for the G workgroups that cooperate on one pair: two buffers
// (alternating by phase), G slots of XCH_WORDS 8-byte {tag, payload} granules.
constexpr int XCH_WORDS = 16;

struct PairDesc {
    const float* fixed;      // two planes of nf float4 (lo_off / hi_off)
    const float* moving;     // two planes of nm float4
    int nf, nm;
    int nf_pad, nm_pad;      // multiples of 64
    int rows_pad;            // rows_per rounded up to 128: row stride of the transposed lists
    int capf;                // flat capacity per row, on average (a workgroup owning r rows may hold r*capf candidates)
    float4* ybuf;            // [G][nm_pad]     transformed moving points {y0,y1,y2,g0} (used when the cloud does not fit in LDS)
    // survivor planes: (nf_pad + G) * capf entries; workgroup g owns [g*rows_per*capf, (g+1)*rows_per*capf)
    // The work buffers below belong to the launch's pair SLOTS, not to the pairs: the pointers are slot 0's, slot s (= blockIdx.x / G)
    // adds s * the strides.  A slot aligns one pair after the other (in-kernel pair queue), so a launch with fewer slots than pairs
    // needs slots x, not pairs x, the memory.
    long long ws_y_stride, ws_list_stride, ws_surv_stride;   // elements per slot of ybuf, of jT (in 16-bit columns) / ent, of surv
    int capn;                // longest row the transposed lists hold (longer => dense fallback)
    uint16_t* jT;            // [G][capn][rows_pad]  the cull's transposed lists: column of entry n of local row li, columns ascending
    uint2* ent;              // same shape, by slot (rows sorted by list length): {colour factor ck as bits (NaN = failed the gate), column}
    uint2* surv;             // nonzeros of A compacted per wave, in the order they were found: {a as bits, slot << 16 | column}
    unsigned long long* xch; // [2][G][XCH_WORDS]
    const PairState* state_in;   // start state: the device copy (carried from the last launch) or a pinned host buffer the caller filled
    PairState* state;            // device copy of the final state
    PairState* state_host;       // pinned host mirror the kernel writes the final state to (no copy engine between launches)
    TraceRow* trace;         // optional
    int trace_cap;
    int* trace_len;
    // Tracker score block in the kernel's tail (cvo::compute_innerproduct, cvo.cpp:475-503, with tran = this alignment's own result and the
    // ell it left behind): non-null = 5 x 24 doubles in pinned host memory, request r at [24 r]: {sum_A, count, 21 Hessian terms}
    // for r = 0 fip(moving, fixed), 1 fip(T moving, fixed), 2 fip(fixed, fixed), 3 fip(moving, moving), 4 se3_Hessian(T moving, fixed);
    // [23] of request 0 = bit mask of the requests the kernel has answered (TAIL_*), the host's score kernel answers the others
    double* score_out;
    const struct SelfCacheEntry* self_fixed;    // the clouds' tables of cached self inner products (ScoreDesc::self_cache)
    const struct SelfCacheEntry* self_moving;
    int run_pair;            // NOT a property of this pair: the pair the launch's position `index of this descriptor` works on (slot s of a launch with a slot per
                             // pair, the s-th pull from the pair queue otherwise).  The host ranks the pairs by the density of their clouds and deals them so
                             // that workgroups sharing an XCD's L2 run pairs of similar density (Engine::launch_impl)
    float* record;           // this pair's 64-byte result record {transform[12], iter, A_nonzero, iterations_run, status as floats}: written by the kernel's
                             // final block, so the cross-GPU gather (or a caller that wants the records on the device) needs no pack kernel behind the launch
    int member_regions;      // adoption launches: member g of a pair keeps its lists and records in a region of its own (sized for the rows it owns
                             // when it joins, at g + 1 members) instead of sharing one region cut into G parts -- see make_ctx
};

// K-stream tracker steps (cvo_tracks_step_async): between the odometry launch and the keyframe launch of a step, cvo_track_link_kernel evaluates
// reset_initial (cvo.cpp:611-618) for every stream whose keyframe object aligns this frame, one lane per stream.  TrackLinkIn: what the keyframe
// object carries, written by the host into pinned memory before the step is queued; TrackLinkOut: what the host takes in when the step is waited for.
struct TrackLinkIn {
    float R[9], T[3], ell;    // the keyframe object's R, T (kept when the odometry alignment failed) and ell
    float transform[12];      // its cvo::transform
    int iter;                 // its iter (Q4: stale unless an alignment breaks)
    int odo_state, key_state; // index of the stream's odometry state (read) and keyframe state (written) in the two engines' state tables
    int pad_;
};
struct TrackLinkOut {
    float R[9], T[3];         // R, T after reset_initial
    float init_inverse[12];   // what reset_initial returns (cvo.cpp:617)
    int odo_status;           // the odometry alignment's status as the kernel read it (CVO_OK: reset_initial was evaluated)
    int pad_[3];
};

// adaptive-ell variant (acvo::align, thirdparty/cvo/src/adaptive_cvo.cpp:490-555)
struct AdaptiveRow { float omega[3], v[3], dl, ell, step; int nnz_xy, nnz_xx, nnz_yy; };   // == cvo_adaptive_row
struct AdaptiveState {
    float R[9], T[3], ell, ell_max, transform[12];
    int iter, iterations_run, status;
    // between the kernels of one iteration
    int stop;                // a stop test fired (or max_iter reached): the kernels still queued return at once
    float M[12];             // this iteration's transform (update_tf)
    float omega[3], v[3], step;
    double dl;
    int nnz_xy, nnz_xx, nnz_yy;
};
struct AdaptiveArgs {
    const float* fixed; const float* moving;   // two planes of float4 each (lo_off / hi_off)
    int nf, nm;
    float4* ybuf;            // nm transformed moving points
    AdaptiveState* state;    // in/out
    double* partials;        // [row blocks][16]: per-workgroup partial sums of a sweep
    AdaptiveRow* trace; int trace_cap; int* trace_len;
    float ell_min, dl_step;
    DevParams P;
};

// score kernels (function_inner_product / se3_Hessian)
struct SelfCacheEntry { float ell; int valid; double sum, count; };
constexpr int SELF_CACHE_N = 4;
struct ScoreDesc {
    const float* a;          // two planes of na float4: queried cloud (positions optionally transformed by tran)
    const float* b;          // two planes of nb float4: searched cloud
    const float* bbox;       // its 32-point group boxes: planes lo x, y, z, y/z then hi x, y, z, y/z of nbox floats each
    int nbox;
    int na, nb;
    float tran[12];
    int use_tran;            // 0: a as stored, 1: a transformed by tran, 2: a transformed by from->transform (the pair's own align() result)
    float ell;
    const PairState* from;   // non-null: ell (and the transform when use_tran == 2) come from this device-resident state, so a score block can be
                             // queued behind the align launch that produces it without a host round trip
    int want_hessian;        // 0: inner product only, 1: Hessian terms too
    double* out;
    // fip(cloud, cloud) of an untransformed cloud against itself depends on the cloud and ell only (cvo.cpp:496-497), and the moving cloud
    // of one frame is the fixed cloud of the next (update_fixed_pcd, cvo.cpp:578-582): non-null = the cloud's table of SELF_CACHE_N
    // entries {ell, valid, sum, count} in HBM (cleared when the cloud's points are written); a hit skips the sweep, a miss fills an entry
    SelfCacheEntry* self_cache;
};

// host clouds in the reference layout -> the two float4 planes (cvo_pack_clouds_kernel): one descriptor per cloud
struct PackDesc {
    unsigned long long raw_off;   // floats from the start of the raw staging buffer: n x 3 positions (AoS, data_type.h:30), then 5 channel-major arrays of n (data_type.h:75)
    float* dst;                   // two planes of n float4
    int n, pad_;
    unsigned long long feat_off;  // floats from the same start to the 5 channel-major feature arrays; 0 = right behind the positions (raw_off + 3 n).  Not 0 for clouds
                                  // handed over in caller-registered memory (cvo_host_register), whose two arrays lie where the caller has them
};

// the batched point-cloud generator (cvo_batch_set_pairs_images): one record per image, zeroed before the select pass, read back by the host
// after the cloud kernel -- the decisions the single-frame path takes on the host (Engine::generate_pcd) stay on the device in between
struct PcdImgRec {
    int sel1[4];                  // n2, n3, n4 of the select pass at potential 3
    int sel2[4];                  // the same for the re-selection
    int pot2;                     // potential of the re-selection, 0 = none (PixelSelector::makeMaps' decision, pcd_decide_kernel)
    int npts;                     // points of the cloud (kept pixels with a valid depth)
    int cost_n, pad_;             // points sampled for cost
    double cost;                  // sum of 1/z^2 over every 16th point with z > 1e-3 (Cloud::cost_hint = cost / cost_n)
    double pad2_;
};
static_assert(sizeof(PcdImgRec) == 64, "PcdImgRec layout");
// pairs' clouds from their images' slots (pcd_scatter_kernel), by value: up to PCD_SCATTER_MAX clouds per launch
constexpr int PCD_SCATTER_MAX = 32;
struct PcdScatter {
    const float* src; const uint16_t* src_px; const PcdImgRec* rec; int cap, n;
    int img[PCD_SCATTER_MAX]; float* dst[PCD_SCATTER_MAX]; uint16_t* dst_px[PCD_SCATTER_MAX];
};

// a caller-owned device image gathered into the generator's packed stacks (pcd_ingest_images_kernel): one descriptor per image, the
// pitches resolved (never 0) and the two read paths decided on the host from these fields alone
struct PcdIngestDesc {
    const uint8_t* bgr;      // pixel (x, y) at bgr + y * bgr_pitch + x * pixel_bytes
    const uint8_t* depth;    // uint16 (x, y) at depth + y * depth_pitch + 2 * x
    long long bgr_pitch, depth_pitch;
    int pixel_bytes, swap_rb;
    int bgr_dwords, depth_dwords;   // base and pitch are multiples of 4: the plane's rows are read as whole dwords (their last, partial dword as bytes)
};
static_assert(sizeof(PcdIngestDesc) == 48, "PcdIngestDesc layout");

// a caller-owned device cloud copied into a cloud's two float4 planes (cvo_ingest_clouds_kernel): one descriptor per cloud, n > 0, the
// strides resolved (never 0) and the read path of the positions decided on the host from these fields alone
struct CloudIngestDesc {
    const float* xyz;        // point i at (const char*)xyz + i * xyz_stride: x, y, z
    const float* feat;       // feature c (0..4) of point i at (const char*)feat + i * feat_point_stride + c * feat_channel_stride
    float* dst;              // two planes of n float4
    double* cost;            // {sum of 1/z^2, samples} per 256-point block of the cloud, in block order (pinned host memory)
    long long xyz_stride, feat_point_stride, feat_channel_stride;   // bytes, multiples of 4
    int n;
    int xyz_tight;           // xyz_stride == 12: a block's positions are consecutive floats, fetched through LDS
};
static_assert(sizeof(CloudIngestDesc) == 64, "CloudIngestDesc layout");

// one cloud of a voxel-grid reduction (cvo_reduce_kernels.hip; not in the reference), n > 0, the strides resolved as in CloudIngestDesc.  The
// scratch arrays lie in the reducer's own memory: an open-addressing table of `slots` cells and what the rows need.
struct ReduceDesc {
    const float* xyz; const float* feat;
    long long xyz_stride, feat_point_stride, feat_channel_stride;
    unsigned long long* keys;      // slots: the cell's 63-bit key, all ones = empty
    unsigned* lowest;              // slots: the lowest member index (atomicMin)
    unsigned* members;             // slots: the member count
    int* row;                      // slots: the cell's output row, -1 = dropped; written for every occupied slot by its lowest member
    int* slot_of;                  // n: the slot of point i's cell, -1 = invalid point
    int* block_heads;              // one per 256 points: the block's kept cells whose lowest member it holds, then their exclusive sum
    int* row_slot;                 // rows_cap: the slot of row r
    long long* sums;               // rows_cap x 8 (MEAN)
    unsigned long long* best;      // rows_cap (CENTRAL): (d2 bits << 32) | index
    float* out_xyz; float* out_feat; int* out_count; int* out_source; int* out_map;   // the caller's arrays; count, source and map may be null
    int* total;                    // the full row count
    int n, slots, cap, rows_cap;   // rows_cap = min(cap, n): rows at or above it are not written
};
static_assert(sizeof(ReduceDesc) == 176, "ReduceDesc layout");
// one (cloud, voxel size) item of a count launch: a table of its own, no rows
struct CountDesc {
    const float* xyz; const float* feat;
    long long xyz_stride, feat_point_stride, feat_channel_stride;
    unsigned long long* keys; unsigned* members; int* total;
    int n, slots; float voxel;
    int src;                       // the item's frame in the launch's frame table (FrameDesc; 0 for a cloud)
};
static_assert(sizeof(CountDesc) == 80, "CountDesc layout");
// one RGB-D frame read in place as a dense cloud (cvo_hip.h, "Reducing frames"; not in the reference): the descriptor of a cvo_device_image with
// the pitches resolved (never 0), the sub-grid and the camera.  A reduction, a count or a fusion of frames has one per frame in a table beside
// its ReduceDesc / CountDesc / FuseMemberDesc records, whose xyz, feat and strides stay 0: point i of the frame is pixel
// ((i % ws) * step, (i / ws) * step), i < ws * ceil(h / step).
struct FrameDesc {
    const uint8_t* bgr;      // pixel (x, y) at bgr + y * bgr_pitch + x * pixel_bytes
    const uint8_t* depth;    // uint16 (x, y) at depth + y * depth_pitch + 2 * x
    long long bgr_pitch, depth_pitch;
    int pixel_bytes, swap_rb;
    int w, h, step, ws;
    float scaling_factor, fx, fy, cx, cy;
    int pad_;
};
static_assert(sizeof(FrameDesc) == 80, "FrameDesc layout");
// one frame of cvo_frames_to_device_clouds: where its dense cloud goes (xyz n x 3, feat n x 5, tight rows)
struct FrameCloudDst { float* xyz; float* feat; };
static_assert(sizeof(FrameCloudDst) == 16, "FrameCloudDst layout");
// one group of a fusion (cvo_fuse_kernels.hip; not in the reference), n > 0: ReduceDesc's scratch arrays over the group's global indices, the
// cells' view masks beside them, and the group's blocks: its members' 256-point blocks one member after the other
struct FuseGroupDesc {
    unsigned long long* keys; unsigned long long* masks;   // slots: the cell's key; the OR of 1 << member number over its members
    unsigned* lowest; unsigned* members;                   // slots: the lowest global member index, the member count
    int* row; int* slot_of; int* block_heads; int* row_slot;   // as ReduceDesc; slot_of per global index, block_heads per block of the group
    long long* sums; unsigned long long* best;             // rows_cap x 8 (MEAN); rows_cap (CENTRAL): (d2 bits << 32) | global index
    float* out_xyz; float* out_feat; int* out_count; int* out_source; int* out_map; int* out_views; unsigned long long* out_view_mask;
    int* total;                    // the full row count
    int n, slots, cap, rows_cap;   // n: the group's points; rows_cap = min(cap, n)
    int n_blocks;                  // the group's blocks
    int first_member, n_members;   // its members with n > 0 in the launch's member table
    int pad_;
};
static_assert(sizeof(FuseGroupDesc) == 176, "FuseGroupDesc layout");
// one member (n > 0) of a group: the grid's second dimension in the passes over points, so no lane searches for its member
struct FuseMemberDesc {
    const float* xyz; const float* feat;
    long long xyz_stride, feat_point_stride, feat_channel_stride;
    float pose[12];                // row-major 3 x 4
    int group;                     // its group in the launch's group table
    int base;                      // the global index of its point 0
    int first_block;               // the group's block number of its block 0
    int n;
    int bit;                       // its member number in the group (empty members counted): the bit it sets in a cell's view mask
    int pad_;
};
static_assert(sizeof(FuseMemberDesc) == 112, "FuseMemberDesc layout");
// one map of a resident-maps call (cvo_map_kernels.hip; not in the reference; cvo_hip.h, "Resident maps"): the grid's second dimension in every
// pass.  A map's rows are a structure of arrays, one array per field, except the 8 sums of a row, which lie together (64 bytes: a wave's rows
// are whole cache lines in the merge's scattered reads and in the extract's dense ones).  The rows exist twice: `to` is where a compaction or a
// restore writes them (the call's host side then swaps the two).  The table maps a cell key to its row: 2 x max_rows slots, open addressing.
struct MapRows {
    unsigned long long* keys;      // the row's cell key
    long long* sums;               // 8 per row
    unsigned* count;
    unsigned long long* mask;      // view_mask
    int* last_stamp; int* born;
};
// where a map lies now: what every kernel that reads or writes a map takes of it (cvo_capi.hip's map_place fills it; the rules that read it
// are cvo_voxel_table.hpp's "a resident map read in place").  A reader that does not use a field leaves it filled; what only a writer uses (`to`)
// lies last, so a reader's uniform loads stay within the record's first 80 bytes.
struct MapPlace {
    MapRows at;                    // the side that holds the rows
    unsigned long long* tkeys; int* trow;   // slots: key (all ones = empty) and row
    int* live;                     // the map's rows with count >= 1
    int rows, slots;               // the map's rows as it stands, dead ones included; the table's size
    MapRows to;                    // the other side: where a compaction or a restore writes the rows
};
// extract's filter (row_kept), which the views and the probes of a map apply as well
struct MapRowFilter { int min_points, min_views, min_last_stamp; };
struct MapDesc : MapPlace {
    int* block_heads;              // one per 256 rows (extract, compact) or per 256 call-cells (an update's births), then their exclusive sum
    int* cell_row;                 // an update: the map row of the call-cell of rank r; -1: absent; after the merge -(row) - 1 for a cell born there
    int* total;                    // the call's figures: [0] rows out (extract, compact) / call-cells, [1] an update's births, [2] its refusal bits
    float* out_xyz; float* out_feat; int* out_count; int* out_views; unsigned long long* out_view_mask;   // extract's arrays, all but xyz, feat may be null
    int* out_last_stamp; int* out_born; int* out_row;
    const uint8_t* drop; int* new_row;   // compact's, either may be null
    int cap;
    int group;                     // an update: its group in the launch's FuseGroupDesc table
    int sign;                      // +1 integrate, -1 remove, -2 remove what is still there (CVO_MAP_*)
    MapRowFilter filter; int probation_from;   // extract's filter / with it compact's keep rule (row_stays)
    int pad_;
    int stamps[64];                // an update: the stamp of member number m of the group
};
static_assert(sizeof(MapRows) == 48 && sizeof(MapPlace) == 128 && sizeof(MapRowFilter) == 12, "MapPlace layout");
static_assert(sizeof(MapDesc) == 520, "MapDesc layout");              // (128 + 24 + 64 + 16 + 32 + 256)
// one view of a viewing call (cvo_view_kernels.hip; not in the reference; cvo_hip.h, "Viewing clouds"): a cloud (n may be 0: its images are
// still written), its pose and camera, its part of the reducer's scratch and the caller's arrays.  The grid's second dimension in every pass.
struct ViewDesc {
    const float* xyz; const float* feat;
    long long xyz_stride, feat_point_stride, feat_channel_stride;
    float pose[12];                // row-major 3 x 4: the cloud's frame to the camera's
    float fx, fy, cx, cy, scaling_factor;
    int n;
    unsigned long long* zbuf;      // gw * gh: the z-cell's least (z' bits << 32) | index, all ones = empty
    int* code;                     // n: the point's z-cell number; -2 valid but not in view; -3 invalid; -4 a map's row that is filtered or dead
    int* block_heads;              // one per 256 points: the block's visible points, then their exclusive sum
    int* block_relations;          // four per 256 points: the block's rows of each relation value (with observed)
    int* total;                    // the full row count, and behind it ...
    int* relation_counts;          // ... the four relation counts over all rows
    const uint8_t* observed;       // uint16 (x, y) at observed + y * observed_pitch + 2 * x; null: no relation
    long long observed_pitch;
    float* out_xyz; float* out_feat; int* out_source; int* out_pixel; int* out_relation; int* out_map; float* out_depth; int* out_index;
    int cap;                       // rows at or above it are not written
    int pad_;
};
static_assert(sizeof(ViewDesc) == 248, "ViewDesc layout");
// the map a view of cvo_maps_view reads in place (cvo_hip.h, "Viewing maps"): one per view, behind the call's ViewDesc records, whose cloud
// fields stay 0 and whose n is the map's rows, dead ones included.  Row r is point r when the filter keeps it.
struct MapViewSrc {
    uint8_t* carve;                // n bytes, or null: 1 where the row is visible with relation 1
    MapRowFilter filter;
    int pad_;
    MapPlace map;
};
static_assert(sizeof(MapViewSrc) == 152, "MapViewSrc layout");
// one probe of a probing call (cvo_probe_kernels.hip; not in the reference; cvo_hip.h, "Probing maps"): a posed member -- a cloud with the
// strides resolved, or a frame read in place (its FrameDesc behind the records, the cloud fields 0) -- and the map it is looked up in, read
// where it lies.  The grid's second dimension.
struct ProbeDesc {
    const float* xyz; const float* feat;
    long long xyz_stride, feat_point_stride, feat_channel_stride;
    float pose[12];                // row-major 3 x 4: the member's frame to the map's
    int n;                         // the member's points
    int reach;                     // 0: the point's own cell; 1: the 27 cells around it
    MapRowFilter filter;
    int pad_;
    int* out_row; float* out_dist2; int* out_count; int* out_views; int* out_last_stamp;   // n each, any may be null
    uint8_t* out_hit;              // map.rows bytes, cleared by the call, or null
    int* block_counts;             // four per 256 points: the block's found, absent, filtered and invalid points
    int* totals;                   // their four sums over the member
    MapPlace map;                  // (last: what the kernel reads of the record ends 256 bytes in, as before the map had a record of its own)
};
static_assert(sizeof(ProbeDesc) == 304, "ProbeDesc layout");
// one map of a snapshot or a restore (cvo_map_snapshot_kernels.hip; not in the reference; cvo_hip.h, "Saving and restoring maps"): the map where
// it lies, the caller's arrays (`ext`: a snapshot's destination, a restore's source) and the call's two figures.  The grid's second dimension.
struct MapSnapDesc : MapPlace {
    MapRows ext;
    int* figures;                  // a restore: [1] the refusal bits
    int ext_rows;                  // a restore: the rows to put in
    int pad_;
};
static_assert(sizeof(MapSnapDesc) == 192, "MapSnapDesc layout");
// one merge of a merging call (cvo_map_merge_kernels.hip; not in the reference; cvo_hip.h, "Merging maps"): the SOURCE map where it lies (it may
// belong to another cvo_maps object: it is only read), which of its rows are kept and by how many bits their cells are shifted.  The grid's
// second dimension in the passes that form the merge's call-cells; the destination is the call's MapDesc of the same number, as in an update.
struct MapMergeDesc : MapPlace {
    MapRowFilter filter;           // extract's filter (row_kept), unless ...
    int all_rows;                  // ... every row is kept, dead ones included
    int level;                     // the destination's voxel is the source's times 2^level: a cell coordinate is shifted right by it
    int group;                     // the merge's FuseGroupDesc in the launch's table: where its call-cells are formed
    int* figures;                  // the destination's figures (MapDesc::total): [2] takes the refusal bit of a cell count that wrapped
};
static_assert(sizeof(MapMergeDesc) == 160, "MapMergeDesc layout");
// what all views of a call share
struct ViewParams {
    int width, height, cell, mode, gw, gh;
    float z_near, z_far, slack, depth_tol;
};

// the group boxes of many clouds in one launch (cvo_cloud_boxes_batch_kernel): one descriptor per cloud, n > 0
struct BoxDesc {
    const float* rec;        // the cloud's two planes of n float4
    float* gbox;             // its boxes: 8 planes of ngroups floats
    SelfCacheEntry* self_cache;   // the cloud's table of cached self inner products (behind the boxes: score_self_cache), emptied by the launch
    int n, ngroups;
};

// One direction of one pair of clouds as the box-culled row sweeps read it (per-point support, point matches): rows and columns are given plane
// by plane, so the rows (or columns) of a transformed cloud are a scratch copy of its {x, y, z, f0} plane beside the cloud's own {f1..f4} plane.
struct SweepSide {
    const float* a_lo; const float* a_hi;   // rows: na float4 {x, y, z, f0} and na float4 {f1, f2, f3, f4}
    const float* b_lo; const float* b_hi;   // columns: nb float4 each
    const float* bbox;                      // boxes of the columns' 32-point groups (of b_lo as it is: planes of nbox floats, as ScoreDesc::bbox)
    int nbox, na, nb;
    float ell;
    const PairState* from;                  // non-null: ell comes from this device-resident state (ScoreDesc::from)
};
static_assert(sizeof(SweepSide) == 64, "SweepSide layout");
// per-point support (cvo_support_kernels.hip; not in the reference): one request of a launch is ONE direction of one pair of clouds -- a {sum, count}
// per ROW over the columns inside both gates.  The table is copied to device memory by the call.
struct SupportDesc : SweepSide {
    float* sum; int* count;                 // na each
};
static_assert(sizeof(SupportDesc) == 80, "SupportDesc layout");
// the pre-pass of a transformed cloud (cvo_support_move_kernel): its {x, y, z, f0} plane with the positions moved, one descriptor per cloud
struct SupportMoveDesc {
    const float* src; float* dst;           // n float4 each
    const PairState* from;                  // non-null: the transform is from->transform (the pair's own align() result), else tran
    float tran[12];
    int n, pad_;
};
static_assert(sizeof(SupportMoveDesc) == 80, "SupportMoveDesc layout");

// point matches (cvo_match_kernels.hip; not in the reference): one request of a launch is ONE direction of one pair of clouds (SweepSide) -- per ROW
// the column of its largest a_ij, that value, the a-weighted mean of its partners' points, and the support's {sum, count}; per request a fit
// record made from those arrays by a second kernel.  The table is copied to device memory by the call.
struct MatchFit { int rows; int matched; double sum_w; double sum_w_res2; };    // cvo_match_fit (include/cvo_hip.h)
static_assert(sizeof(MatchFit) == 24, "MatchFit layout");
struct MatchDesc : SweepSide {
    int* best; float* best_value;           // na each
    float* mean;                            // na x 3
    float* sum; int* count;                 // na each
    MatchFit* fit;                          // null: no fit record for this request
};
static_assert(sizeof(MatchDesc) == 112, "MatchDesc layout");

// pose hypotheses (cvo_hypothesis_kernels.hip; not in the reference): one pair of a launch -- its moving cloud under each of the launch's K transforms
// against its fixed cloud, function_inner_product's sum per transform.  The table and the transforms are copied to device memory by the call.
struct HypDesc {
    const float* a;                         // moving cloud: two planes of na float4 (lo_off / hi_off)
    const float* b;                         // fixed cloud: two planes of nb float4
    const float* bbox;                      // boxes of b's 32-point groups (planes of nbox floats, as ScoreDesc::bbox)
    const float* trans;                     // this pair's K transforms, 12 floats each (moving -> fixed, 3x4 row-major)
    PairState* state;                       // seeding: the pair's device-resident state, written by the select step; null = scores only
    int nbox, na, nb;
    float ell;
    float seed_ell; int seed_iter;          // seeding: what the state takes from the pair's start state besides R, T (cvo_track_link_kernel's TrackLinkIn)
    float seed_transform[12];
};
static_assert(sizeof(HypDesc) == 112, "HypDesc layout");
struct HypScore { float value; int num; int num_e; };   // == cvo_inn_p (include/cvo_hip.h)

// pose models (cvo_pose_model_kernels.hip; not in the reference): one pair of a launch -- value, se(3) gradient and Hessian of that sum at each of the
// launch's K transforms.  HypDesc without the seeding fields, and with the state a result call reads its one transform and its ell from.
struct PoseModelDesc {
    const float* a;                         // moving cloud: two planes of na float4 (lo_off / hi_off)
    const float* b;                         // fixed cloud: two planes of nb float4
    const float* bbox;                      // boxes of b's 32-point groups (planes of nbox floats, as ScoreDesc::bbox)
    const float* trans;                     // this pair's K transforms, 12 floats each (moving -> fixed, 3x4 row-major); unused with `from`
    const PairState* from;                  // non-null (K = 1): the transform is from->transform and ell is from->ell (the pair's own align() result)
    int nbox, na, nb;
    float ell;
};
static_assert(sizeof(PoseModelDesc) == 56, "PoseModelDesc layout");
constexpr int POSE_MODEL_TERMS = 29;        // a block's record of doubles: sum, count, 6 gradient sums, the 21 sums of pair_hessian_add_weighted
struct PoseModel { float value; int num; double grad[6]; double hess[36]; };   // == cvo_pose_model (include/cvo_hip.h)
static_assert(sizeof(PoseModel) == 344, "PoseModel layout");

// a score block: up to 8 inner-product / Hessian requests evaluated by one launch
constexpr int SCORE_MAXREQ = 8;
struct ScoreBatch {
    ScoreDesc d[SCORE_MAXREQ];
    int n;
};

}  // namespace cvohip
