// cvo_reduce_kernels.hip -- voxel-grid reduction of caller-owned device clouds to a point budget (NOT in the reference): the front end of the
// device-cloud hand-over (cvo_device_cloud).  The definition is include/cvo_hip.h's "Reducing clouds" (tests/voxel_reading.py restates it in
// numpy); every output is held to it bit for bit.  The seven passes, the table and the runs of lanes are cvo_voxel_table.hpp's; this file gives
// them a record per cloud, and adds the count kernels and the dense clouds of frames.
//
// A point's cell is the triple c = floorf(x / voxel) of its position, |c| < 2^20, packed with an offset of 2^20 into 63 bits.  Each cloud of a
// call has an open-addressing table of slots = 2 n cells (linear probing, at most half full, so an insert always ends) in the reducer's scratch.
// All clouds of a call run together: every kernel's grid has the cloud in its second dimension, as cvo_ingest_clouds_kernel, and a block whose
// first point lies past its cloud's n leaves at once.  A lane reads a point's floats for i < n only: the extents the host has checked.  A
// point's index is its index in the cloud, its block's number blockIdx.x.  With 307200-point depth clouds at 3072 rows the runs of lanes took
// the reduction from 12.6 to the figures in profiles/reduce_clouds.txt.
// cvo_count_voxels runs clear + insert alone over (cloud, voxel size) items, each with a table of its own: with min_points == 1 a cell is
// counted by the lane whose compare-and-swap claimed its slot, otherwise by the lane whose atomicAdd brought `members` to min_points -- one
// lane per counted cell either way; a block adds its lanes with __syncthreads_count and does one atomicAdd into the item's total.
//
// Point sources.  The passes that read points -- insert, gather, CENTRAL's write, count-insert -- take the source as a template parameter
// (cvo_voxel_table.hpp): CloudSource reads a cvo_device_cloud's arrays; FrameSource computes the point of a sub-grid pixel of an RGB-D frame
// where it is needed (cvo_hip.h, "Reducing frames"), so a frame is reduced without a dense cloud in memory: insert and count-insert read the
// pixel's depth alone (2 bytes; a frame's features cannot be invalid), gather recomputes position and features from the pixel and its four
// flat neighbours (bytes another lane of the block has just read), the write recomputes the winner.  clear, heads, offsets and rows read no
// point and have one form.  cvo_frames_to_clouds_kernel writes the dense clouds themselves for callers that want them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"   // the point sources, the table and the passes: shared with cvo_fuse_kernels.hip

namespace cvohip {
namespace {
struct Nothing { template <class... A> __device__ __forceinline__ void operator()(A...) const {} };
struct Kept { __device__ __forceinline__ bool operator()(int) const { return true; } };   // (min_points alone decides)
}  // namespace

__global__ __launch_bounds__(RB) void cvo_reduce_clear_kernel(const ReduceDesc* __restrict__ descs) {
    clear_pass(descs[blockIdx.y], (long long)blockIdx.x * RB + threadIdx.x, Nothing());
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_reduce_insert_kernel(const ReduceDesc* __restrict__ descs, typename Src::Table T, float voxel) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    u64 key = KEY_EMPTY;                                              // (an invalid point, or none: no cell)
    if (i < D.n) {
        float v[8], c[3];
        point_for_cell<Src>(D, T, blockIdx.y, i, v);
        if (!cell_of(v, voxel, c, &key)) key = KEY_EMPTY;
    }
    bool run_tail;
    const int s = insert_pass(D, key, (unsigned)i, lane, &run_tail);
    if (i < D.n) D.slot_of[i] = s;
}
__global__ __launch_bounds__(RB) void cvo_reduce_heads_kernel(const ReduceDesc* __restrict__ descs, int min_points) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block)
    const int s = i < D.n ? D.slot_of[i] : -1;
    const int k = __syncthreads_count(head_of(D, i, s, min_points, Kept()) == 1);
    if (threadIdx.x == 0) D.block_heads[blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_reduce_offsets_kernel(const ReduceDesc* __restrict__ descs) {
    const ReduceDesc& D = descs[blockIdx.y];
    offsets_pass(D, (D.n + RB - 1) / RB);
}
__global__ __launch_bounds__(RB) void cvo_reduce_rows_kernel(const ReduceDesc* __restrict__ descs, int min_points) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block)
    const int s = i < D.n ? D.slot_of[i] : -1;
    rows_pass(D, blockIdx.x, head_of(D, i, s, min_points, Kept()), s);
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_reduce_gather_kernel(const ReduceDesc* __restrict__ descs, typename Src::Table T, float voxel, int mode) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    const int r = row_of_point(D, i < D.n, i);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 0) Src::point(D, T, blockIdx.y, i, v);
    gather_pass(D, r, v, (unsigned)i, lane, voxel, mode);
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_reduce_write_kernel(const ReduceDesc* __restrict__ descs, typename Src::Table T, int mode) {
    const ReduceDesc& D = descs[blockIdx.y];
    write_pass(D, blockIdx.x * RB + threadIdx.x, mode, [&](unsigned src, int k) {   // the winner as it lies in the cloud
        if (k >= 3) return Src::feature(D, T, blockIdx.y, (long long)src, k - 3);
        float p[3];
        Src::position(D, T, blockIdx.y, (int)src, p);
        return k == 0 ? p[0] : k == 1 ? p[1] : p[2];
    }, Nothing());
}

__global__ __launch_bounds__(RB) void cvo_count_clear_kernel(const CountDesc* __restrict__ descs) {
    const CountDesc& D = descs[blockIdx.y];
    const long long g = (long long)blockIdx.x * RB + threadIdx.x;
    if (g < D.slots) { D.keys[g] = KEY_EMPTY; D.members[g] = 0u; }
    if (g == 0) *D.total = 0;
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_count_insert_kernel(const CountDesc* __restrict__ descs, typename Src::Table T, int min_points) {
    const CountDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block)
    u64 key = KEY_EMPTY;
    if (i < D.n) {
        float v[8], c[3];
        point_for_cell<Src>(D, T, D.src, i, v);
        if (!cell_of(v, D.voxel, c, &key)) key = KEY_EMPTY;
    }
    int start; bool tail, counted = false;
    lane_runs(key, lane, &start, &tail);
    if (key != KEY_EMPTY && tail) {                                   // one insert per run, with the run's length
        bool fresh;
        const unsigned s = table_insert(D.keys, (unsigned)D.slots, key, &fresh);
        if (min_points == 1) counted = fresh;
        else {
            const unsigned len = (unsigned)(lane - start + 1), before = atomicAdd(&D.members[s], len);
            counted = before < (unsigned)min_points && before + len >= (unsigned)min_points;
        }
    }
    const int k = __syncthreads_count(counted);
    if (threadIdx.x == 0 && k) atomicAdd(D.total, k);
}

// the dense clouds of frames themselves (cvo_frames_to_device_clouds): a lane per sub-grid pixel writes its point's 8 floats
__global__ __launch_bounds__(RB) void cvo_frames_to_clouds_kernel(const FrameDesc* __restrict__ frames, const FrameCloudDst* __restrict__ dst, int n) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const FrameSource::Table T = {frames};
    const FrameCloudDst O = dst[blockIdx.y];
    float v[8];
    FrameSource::point(O, T, blockIdx.y, i, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) O.xyz[3 * (size_t)i + k] = v[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) O.feat[5 * (size_t)i + k] = v[3 + k];
}

namespace {
// descs: the device's copy of the table, every cloud with n > 0.  n_max, slots_max, rows_max: the largest n, slots and rows_cap among them.
template <class Src>
hipError_t launch_reduce(const ReduceDesc* descs, typename Src::Table T, int n_clouds, int n_max, int slots_max, int rows_max, float voxel, int mode,
                         int min_points, hipStream_t s) {
    if (n_clouds <= 0 || n_max <= 0) return hipSuccess;
    const dim3 blk(RB), pts((n_max + RB - 1) / RB, n_clouds);
    const long long clear = slots_max > 8ll * rows_max ? slots_max : 8ll * rows_max;
    hipLaunchKernelGGL(cvo_reduce_clear_kernel, dim3((unsigned)((clear + RB - 1) / RB), n_clouds), blk, 0, s, descs);
    hipLaunchKernelGGL(cvo_reduce_insert_kernel<Src>, pts, blk, 0, s, descs, T, voxel);
    hipLaunchKernelGGL(cvo_reduce_heads_kernel, pts, blk, 0, s, descs, min_points);
    hipLaunchKernelGGL(cvo_reduce_offsets_kernel, dim3(1, n_clouds), blk, 0, s, descs);
    hipLaunchKernelGGL(cvo_reduce_rows_kernel, pts, blk, 0, s, descs, min_points);
    hipLaunchKernelGGL(cvo_reduce_gather_kernel<Src>, pts, blk, 0, s, descs, T, voxel, mode);
    if (rows_max > 0) hipLaunchKernelGGL(cvo_reduce_write_kernel<Src>, dim3((8 * rows_max + RB - 1) / RB, n_clouds), blk, 0, s, descs, T, mode);
    return hipGetLastError();
}
template <class Src>
hipError_t launch_count(const CountDesc* descs, typename Src::Table T, int n_items, int n_max, int slots_max, int min_points, hipStream_t s) {
    if (n_items <= 0 || n_max <= 0) return hipSuccess;
    hipLaunchKernelGGL(cvo_count_clear_kernel, dim3((slots_max + RB - 1) / RB, n_items), dim3(RB), 0, s, descs);
    hipLaunchKernelGGL(cvo_count_insert_kernel<Src>, dim3((n_max + RB - 1) / RB, n_items), dim3(RB), 0, s, descs, T, min_points);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_reduce_clouds(const ReduceDesc* descs, int n_clouds, int n_max, int slots_max, int rows_max, float voxel, int mode, int min_points,
                                hipStream_t s) {
    return launch_reduce<CloudSource>(descs, CloudSource::Table(), n_clouds, n_max, slots_max, rows_max, voxel, mode, min_points, s);
}
hipError_t launch_count_voxels(const CountDesc* descs, int n_items, int n_max, int slots_max, int min_points, hipStream_t s) {
    return launch_count<CloudSource>(descs, CloudSource::Table(), n_items, n_max, slots_max, min_points, s);
}
// the same over frames read in place: frames[q] is the frame of descs[q] (a reduction) or of descs[q].src (a count)
hipError_t launch_reduce_frames(const ReduceDesc* descs, const FrameDesc* frames, int n_frames, int n, int rows_max, float voxel, int mode, int min_points,
                                hipStream_t s) {
    const FrameSource::Table T = {frames};
    return launch_reduce<FrameSource>(descs, T, n_frames, n, 2 * n, rows_max, voxel, mode, min_points, s);
}
hipError_t launch_count_frame_voxels(const CountDesc* descs, const FrameDesc* frames, int n_items, int n, int min_points, hipStream_t s) {
    const FrameSource::Table T = {frames};
    return launch_count<FrameSource>(descs, T, n_items, n, 2 * n, min_points, s);
}
hipError_t launch_frames_to_clouds(const FrameDesc* frames, const FrameCloudDst* dst, int n_frames, int n, hipStream_t s) {
    if (n_frames <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cvo_frames_to_clouds_kernel, dim3((n + RB - 1) / RB, n_frames), dim3(RB), 0, s, frames, dst, n);
    return hipGetLastError();
}
}  // namespace cvohip
