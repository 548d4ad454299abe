// cvo_reduce_kernels.hip -- voxel-grid reduction of caller-owned device clouds to a point budget (NOT in the reference): the front end of the
// device-cloud hand-over (cvo_device_cloud).  The definition is include/cvo_hip.h's "Reducing clouds" (tests/voxel_reading.py restates it in
// numpy); every output is held to it bit for bit, so every value that reaches an output is independent of the order in which points arrive:
// integer atomicAdd / atomicMin / compare-and-swap of a key only, no float atomics, and the place of a cell in the table never shows.
//
// A point's cell is the triple c = floorf(x / voxel) of its position, |c| < 2^20, packed with an offset of 2^20 into 63 bits.  Each cloud of a
// call has an open-addressing table of slots = 2 n cells (linear probing, at most half full, so an insert always ends) in the reducer's scratch.
// All clouds of a call run together: every kernel's grid has the cloud in its second dimension, as cvo_ingest_clouds_kernel, and a block whose
// first point lies past its cloud's n leaves at once.  A lane reads a point's floats for i < n only: the extents the host has checked.
//
// The launches of one reduction, in stream order:
//   clear    the table's keys to empty, lowest to all ones, members to 0; the rows' sums to 0 and bests to all ones
//   insert   a lane per point: validity, key, CAS-insert; atomicMin of the point's index into the slot's `lowest`, atomicAdd of 1 into its
//            `members`; the point's slot (-1: invalid) is kept for the later passes
//   heads    a block per 256 points counts its heads: points that are their cell's lowest member in a cell with at least min_points members
//   offsets  a block per cloud turns the blocks' counts into their exclusive sums and writes the cloud's row count
//   rows     a head's row is its block's offset + the heads before it in the block: rows ascend with the lowest member index.  The head writes
//            the row into its slot (-1 for the lowest member of a dropped cell), and the slot into row_slot[row] for rows below cap
//   gather   a lane per point again: map[i] = its cell's row; for rows below cap, MEAN adds q = llrint((double)v * 2^24) of its 8 values into
//            the row's 64-bit sums (|v| < 2^15 and n < 2^20: below 2^59), CENTRAL does a 64-bit atomicMin of (d2 bits << 32) | i
//   write    a lane per (row, value): MEAN (float)((double)sum / ((double)count * 16777216.0)), CENTRAL the value of the winning member
// Runs: neighbouring points of a dense cloud mostly share a cell, so in insert and gather a run of consecutive lanes of a wave with one cell acts
// once -- its first lane inserts and gives its index to `lowest`, its last lane adds the run's length to `members`, the run's q (or its least
// (d2, index)) are combined with a segmented scan over __shfl_up and its last lane does the atomics.  Integer sums and minima: the same bits as
// a lane-by-lane form.  With 307200-point depth clouds at 3072 rows this took the reduction from 12.6 to the figures in profiles/reduce_clouds.txt.
// cvo_count_voxels runs clear + insert alone over (cloud, voxel size) items, each with a table of its own: with min_points == 1 a cell is
// counted by the lane whose compare-and-swap claimed its slot, otherwise by the lane whose atomicAdd brought `members` to min_points -- one
// lane per counted cell either way; a block adds its lanes with __syncthreads_count and does one atomicAdd into the item's total.
//
// Point sources.  The passes that read points -- insert, gather, CENTRAL's write, count-insert -- take the source as a template parameter
// (cvo_voxel_table.hpp): CloudSource reads a cvo_device_cloud's arrays as before; FrameSource computes the point of a sub-grid pixel of an RGB-D
// frame where it is needed (cvo_hip.h, "Reducing frames"), so a frame is reduced without a dense cloud in memory: insert and count-insert read
// the pixel's depth alone (2 bytes; a frame's features cannot be invalid), gather recomputes position and features from the pixel and its four
// flat neighbours (bytes another lane of the block has just read), the write recomputes the winner.  clear, heads, offsets and rows read no
// point and have one form.  cvo_frames_to_clouds_kernel writes the dense clouds themselves for callers that want them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"   // load_point, cell_of, table_insert, lane_runs: shared with cvo_fuse_kernels.hip

namespace cvohip {
namespace {
// is point i (i < n) the lowest member of a kept cell / of a dropped one
__device__ __forceinline__ void head_of(const ReduceDesc& D, int i, int min_points, int* slot, bool* head, bool* dropped) {
    const int s = D.slot_of[i];
    *slot = s; *head = false; *dropped = false;
    if (s < 0 || D.lowest[s] != (unsigned)i) return;
    if (D.members[s] >= (unsigned)min_points) *head = true; else *dropped = true;
}
}  // namespace

__global__ __launch_bounds__(RB) void cvo_reduce_clear_kernel(const ReduceDesc* __restrict__ descs) {
    const ReduceDesc& D = descs[blockIdx.y];
    const long long g = (long long)blockIdx.x * RB + threadIdx.x;
    if (g < D.slots) { D.keys[g] = KEY_EMPTY; D.lowest[g] = 0xFFFFFFFFu; D.members[g] = 0u; }
    if (g < 8ll * D.rows_cap) D.sums[g] = 0;
    if (g < D.rows_cap) D.best[g] = KEY_EMPTY;
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
    int start; bool tail, fresh;
    lane_runs(key, lane, &start, &tail);
    int s = -1;
    if (key != KEY_EMPTY && lane == start) {                          // a run's first lane holds its lowest index
        s = (int)table_insert(D.keys, (unsigned)D.slots, key, &fresh);
        atomicMin(&D.lowest[s], (unsigned)i);
    }
    s = __shfl(s, start);
    if (key != KEY_EMPTY && tail) atomicAdd(&D.members[s], (unsigned)(lane - start + 1));
    if (i < D.n) D.slot_of[i] = s;
}
__global__ __launch_bounds__(RB) void cvo_reduce_heads_kernel(const ReduceDesc* __restrict__ descs, int min_points) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block)
    int s; bool head = false, dropped;
    if (i < D.n) head_of(D, i, min_points, &s, &head, &dropped);
    const int k = __syncthreads_count(head);
    if (threadIdx.x == 0) D.block_heads[blockIdx.x] = k;
}
// one block per cloud: thread t owns `per` consecutive blocks' counts; their sums are scanned through LDS
__global__ __launch_bounds__(RB) void cvo_reduce_offsets_kernel(const ReduceDesc* __restrict__ descs) {
    __shared__ int part[RB];
    const ReduceDesc& D = descs[blockIdx.y];
    const int nb = (D.n + RB - 1) / RB, per = (nb + RB - 1) / RB, t = threadIdx.x;
    const int from = min(nb, t * per), to = min(nb, from + per);
    int sum = 0;
    for (int j = from; j < to; ++j) sum += D.block_heads[j];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < RB; d <<= 1) {
        const int add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int at = part[t] - sum;
    for (int j = from; j < to; ++j) { const int k = D.block_heads[j]; D.block_heads[j] = at; at += k; }
    if (t == RB - 1) *D.total = part[t];
}
__global__ __launch_bounds__(RB) void cvo_reduce_rows_kernel(const ReduceDesc* __restrict__ descs, int min_points) {
    __shared__ int wave_heads[RB / 64];
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block)
    int s = -1; bool head = false, dropped = false;
    if (i < D.n) head_of(D, i, min_points, &s, &head, &dropped);
    const u64 b = __ballot(head);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_heads[w] = __popcll(b);
    __syncthreads();
    if (dropped) D.row[s] = -1;
    if (head) {
        int r = D.block_heads[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; ++q) r += wave_heads[q];
        D.row[s] = r;
        if (r < D.rows_cap) D.row_slot[r] = s;
    }
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_reduce_gather_kernel(const ReduceDesc* __restrict__ descs, typename Src::Table T, float voxel, int mode) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= D.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    int r = -1;                                                       // the point's row if it is one that is written
    if (i < D.n) {
        const int s = D.slot_of[i];
        r = s >= 0 ? D.row[s] : -1;
        if (D.out_map) D.out_map[i] = r;
        if (r >= D.rows_cap) r = -1;
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 0) Src::point(D, T, blockIdx.y, i, v);
    if (mode == 0) {                                                  // CVO_REDUCE_MEAN: a run of lanes with one row adds its q on chip (integers: any order gives the same sum)
        u64 q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = (u64)__double2ll_rn((double)v[k] * 16777216.0);   // (two's complement: the signed sum)
        int start; bool tail;
        lane_runs(r, lane, &start, &tail);
        for (int d = 1; d < 64; d <<= 1) {                            // segmented inclusive scan: a run's last lane ends with the run's sums
            const bool take = lane - d >= start;
            if (__ballot(take) == 0ull) break;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const u64 up = __shfl_up(q[k], d); if (take) q[k] += up; }
        }
        if (r >= 0 && tail) {
            u64* sums = reinterpret_cast<u64*>(D.sums) + 8 * (size_t)r;
#pragma unroll
            for (int k = 0; k < 8; ++k) atomicAdd(&sums[k], q[k]);
        }
    } else {                                                          // CVO_REDUCE_CENTRAL: a run's least (d2 bits, index) the same way
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = floorf(__fdiv_rn(v[k], voxel));
            const float d = __fsub_rn(v[k], __fmul_rn(__fadd_rn(c, 0.5f), voxel));
            d2 = k == 0 ? __fmul_rn(d, d) : __fadd_rn(d2, __fmul_rn(d, d));
        }
        u64 best = r >= 0 ? ((u64)__float_as_uint(d2) << 32) | (u64)(unsigned)i : KEY_EMPTY;
        int start; bool tail;
        lane_runs(r, lane, &start, &tail);
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= start;
            if (__ballot(take) == 0ull) break;
            const u64 up = __shfl_up(best, d);
            if (take && up < best) best = up;
        }
        if (r >= 0 && tail) atomicMin(&D.best[r], best);
    }
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_reduce_write_kernel(const ReduceDesc* __restrict__ descs, typename Src::Table T, int mode) {
    const ReduceDesc& D = descs[blockIdx.y];
    const int g = blockIdx.x * RB + threadIdx.x, r = g >> 3, k = g & 7;
    if (r >= min(*D.total, D.rows_cap)) return;
    const int s = D.row_slot[r];
    const unsigned cnt = D.members[s];
    unsigned src; float val;
    if (mode == 0) {
        src = D.lowest[s];
        val = (float)((double)D.sums[g] / ((double)cnt * 16777216.0));
    } else {
        src = (unsigned)(D.best[r] & 0xFFFFFFFFull);
        if (k < 3) {
            float p[3];
            Src::position(D, T, blockIdx.y, (int)src, p);
            val = k == 0 ? p[0] : k == 1 ? p[1] : p[2];
        } else {
            val = Src::feature(D, T, blockIdx.y, (long long)src, k - 3);
        }
    }
    if (k < 3) D.out_xyz[3 * (size_t)r + k] = val; else D.out_feat[5 * (size_t)r + (k - 3)] = val;
    if (k == 0) {
        if (D.out_count) D.out_count[r] = (int)cnt;
        if (D.out_source) D.out_source[r] = (int)src;
    }
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
