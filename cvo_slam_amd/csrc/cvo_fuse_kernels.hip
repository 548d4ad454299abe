// cvo_fuse_kernels.hip -- fusing posed device clouds into voxel-reduced local maps (NOT in the reference): the reducer's table, row ranking and
// order-free integer sums (cvo_reduce_kernels.hip) over a GROUP of clouds, each under its pose.  The definition is include/cvo_hip.h's "Fusing
// clouds" (tests/fuse_reading.py restates it in numpy): a fusion is the reduction of the concatenation of the moved members, plus the views
// filter and the two view outputs; every output is held to it bit for bit.
//
// The group's points have global indices: member after member.  A group has ONE table (slots = 2 x its points) and one set of rows; the passes
// over points have the MEMBER in the grid's second dimension, so all lanes of a block belong to one member, read one pose (uniform loads) and
// never search for their member.  A member's 256-point blocks have consecutive block numbers in its group (first_block + blockIdx.x), members in
// order: the heads / offsets / rows passes rank by global index exactly as the reducer ranks by index.
//
// A point's moved position is x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3] by __fmul_rn / __fadd_rn: no contraction, the same bits wherever it
// is computed again (insert, gather, and the CENTRAL write of the winner).  Valid: the 8 source floats and the 3 moved ones finite and below
// 2^15, the cell coordinates of the moved position below 2^20.
//
// The launches of one fusion, in stream order -- seven, whatever the numbers of groups and members:
//   clear    the reducer's, and the view masks to 0
//   insert   a lane per point: move, validity, key, CAS-insert, atomicMin of the global index into `lowest`, atomicAdd into `members`, atomicOr of
//            the member's bit into the slot's view mask -- each once per run of lanes with one cell, as in the reducer
//   heads    a block counts its heads: lowest members of cells with at least min_points members AND at least min_views set bits
//   offsets  a block per group: exclusive sums over the group's blocks, the row count
//   rows     heads take their rows; the lowest member of a dropped cell writes -1
//   gather   map[g]; MEAN adds q = llrint((double)v * 2^24) of the moved position and the features, CENTRAL takes the least (d2 bits, g)
//   write    a lane per (row, value); views and view_mask beside count and source
// Integer atomics only (add, min, or, compare-and-swap of a key).
// insert, gather and write take the point source as a template parameter, as the reducer's passes do (cvo_voxel_table.hpp): a member is a
// cvo_device_cloud (CloudSource) or an RGB-D frame read in place (FrameSource, member q's frame at frames[q]; cvo_fuse_device_frames).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
// rows 0 .. 2 of the moved position; the features pass through
__device__ __forceinline__ float move_row(const float* M, int r, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(M[4 * r], x), __fadd_rn(__fmul_rn(M[4 * r + 1], y), __fmul_rn(M[4 * r + 2], z))), M[4 * r + 3]);
}
// member point i (i < n): its source floats v, and w = (moved position, features); for_cell: what validity and cell need (point_for_cell)
template <class Src>
__device__ __forceinline__ void load_moved(const FuseMemberDesc& M, typename Src::Table T, int which, int i, bool for_cell, float v[8], float w[8]) {
    if (for_cell) point_for_cell<Src>(M, T, which, i, v); else Src::point(M, T, which, i, v);
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = move_row(M.pose, r, v[0], v[1], v[2]);
#pragma unroll
    for (int k = 3; k < 8; ++k) w[k] = v[k];
}
// is global index g, in slot s, the lowest member of a kept cell (1) / of a dropped one (2); 0: neither
__device__ __forceinline__ int fuse_head_of(const FuseGroupDesc& G, int g, int s, int min_points, int min_views) {
    if (s < 0 || G.lowest[s] != (unsigned)g) return 0;
    return G.members[s] >= (unsigned)min_points && __popcll(G.masks[s]) >= min_views ? 1 : 2;
}
}  // namespace

__global__ __launch_bounds__(RB) void cvo_fuse_clear_kernel(const FuseGroupDesc* __restrict__ groups) {
    const FuseGroupDesc& G = groups[blockIdx.y];
    const long long g = (long long)blockIdx.x * RB + threadIdx.x;
    if (g < G.slots) { G.keys[g] = KEY_EMPTY; G.masks[g] = 0ull; G.lowest[g] = 0xFFFFFFFFu; G.members[g] = 0u; }
    if (g < 8ll * G.rows_cap) G.sums[g] = 0;
    if (g < G.rows_cap) G.best[g] = KEY_EMPTY;
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_fuse_insert_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, typename Src::Table T,
                                                             float voxel) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    const FuseGroupDesc& G = groups[M.group];
    u64 key = KEY_EMPTY;                                              // (an invalid point, or none: no cell)
    if (i < M.n) {
        float v[8], w[8], c[3];
        load_moved<Src>(M, T, blockIdx.y, i, true, v, w);
        const bool src_ok = fabsf(v[0]) < 32768.f && fabsf(v[1]) < 32768.f && fabsf(v[2]) < 32768.f;   // (the features are w's)
        if (!cell_of(w, voxel, c, &key) || !src_ok) key = KEY_EMPTY;
    }
    int start; bool tail, fresh;
    lane_runs(key, lane, &start, &tail);
    int s = -1;
    if (key != KEY_EMPTY && lane == start) {                          // a run's first lane holds its lowest index
        s = (int)table_insert(G.keys, (unsigned)G.slots, key, &fresh);
        atomicMin(&G.lowest[s], (unsigned)(M.base + i));
    }
    s = __shfl(s, start);
    if (key != KEY_EMPTY && tail) {
        atomicAdd(&G.members[s], (unsigned)(lane - start + 1));
        atomicOr(&G.masks[s], 1ull << M.bit);
    }
    if (i < M.n) G.slot_of[M.base + i] = s;
}
__global__ __launch_bounds__(RB) void cvo_fuse_heads_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, int min_points, int min_views) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block)
    const FuseGroupDesc& G = groups[M.group];
    const int s = i < M.n ? G.slot_of[M.base + i] : -1;
    const int k = __syncthreads_count(fuse_head_of(G, M.base + i, s, min_points, min_views) == 1);
    if (threadIdx.x == 0) G.block_heads[M.first_block + blockIdx.x] = k;
}
// one block per group: thread t owns `per` consecutive blocks' counts; their sums are scanned through LDS (the reducer's, over n_blocks)
__global__ __launch_bounds__(RB) void cvo_fuse_offsets_kernel(const FuseGroupDesc* __restrict__ groups) {
    __shared__ int part[RB];
    const FuseGroupDesc& G = groups[blockIdx.y];
    const int nb = G.n_blocks, per = (nb + RB - 1) / RB, t = threadIdx.x;
    const int from = min(nb, t * per), to = min(nb, from + per);
    int sum = 0;
    for (int j = from; j < to; ++j) sum += G.block_heads[j];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < RB; d <<= 1) {
        const int add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int at = part[t] - sum;
    for (int j = from; j < to; ++j) { const int k = G.block_heads[j]; G.block_heads[j] = at; at += k; }
    if (t == RB - 1) *G.total = part[t];
}
__global__ __launch_bounds__(RB) void cvo_fuse_rows_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, int min_points, int min_views) {
    __shared__ int wave_heads[RB / 64];
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block)
    const FuseGroupDesc& G = groups[M.group];
    const int s = i < M.n ? G.slot_of[M.base + i] : -1;
    const int what = fuse_head_of(G, M.base + i, s, min_points, min_views);
    const bool head = what == 1, dropped = what == 2;
    const u64 b = __ballot(head);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_heads[w] = __popcll(b);
    __syncthreads();
    if (dropped) G.row[s] = -1;
    if (head) {
        int r = G.block_heads[M.first_block + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; ++q) r += wave_heads[q];
        G.row[s] = r;
        if (r < G.rows_cap) G.row_slot[r] = s;
    }
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_fuse_gather_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, typename Src::Table T,
                                                             float voxel, int mode) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    const FuseGroupDesc& G = groups[M.group];
    const int g = M.base + i;
    int r = -1;                                                       // the point's row if it is one that is written
    if (i < M.n) {
        const int s = G.slot_of[g];
        r = s >= 0 ? G.row[s] : -1;
        if (G.out_map) G.out_map[g] = r;
        if (r >= G.rows_cap) r = -1;
    }
    float v[8], w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 0) load_moved<Src>(M, T, blockIdx.y, i, false, v, w);
    if (mode == 0) {                                                  // CVO_REDUCE_MEAN: a run of lanes with one row adds its q on chip (integers: any order gives the same sum)
        u64 q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = (u64)__double2ll_rn((double)w[k] * 16777216.0);   // (two's complement: the signed sum)
        int start; bool tail;
        lane_runs(r, lane, &start, &tail);
        for (int d = 1; d < 64; d <<= 1) {                            // segmented inclusive scan: a run's last lane ends with the run's sums
            const bool take = lane - d >= start;
            if (__ballot(take) == 0ull) break;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const u64 up = __shfl_up(q[k], d); if (take) q[k] += up; }
        }
        if (r >= 0 && tail) {
            u64* sums = reinterpret_cast<u64*>(G.sums) + 8 * (size_t)r;
#pragma unroll
            for (int k = 0; k < 8; ++k) atomicAdd(&sums[k], q[k]);
        }
    } else {                                                          // CVO_REDUCE_CENTRAL: a run's least (d2 bits, global index) the same way
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = floorf(__fdiv_rn(w[k], voxel));
            const float d = __fsub_rn(w[k], __fmul_rn(__fadd_rn(c, 0.5f), voxel));
            d2 = k == 0 ? __fmul_rn(d, d) : __fadd_rn(d2, __fmul_rn(d, d));
        }
        u64 best = r >= 0 ? ((u64)__float_as_uint(d2) << 32) | (u64)(unsigned)g : KEY_EMPTY;
        int start; bool tail;
        lane_runs(r, lane, &start, &tail);
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= start;
            if (__ballot(take) == 0ull) break;
            const u64 up = __shfl_up(best, d);
            if (take && up < best) best = up;
        }
        if (r >= 0 && tail) atomicMin(&G.best[r], best);
    }
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_fuse_write_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, typename Src::Table T,
                                                            int mode) {
    const FuseGroupDesc& G = groups[blockIdx.y];
    const int g = blockIdx.x * RB + threadIdx.x, r = g >> 3, k = g & 7;
    if (r >= min(*G.total, G.rows_cap)) return;
    const int s = G.row_slot[r];
    const unsigned cnt = G.members[s];
    unsigned src; float val;
    if (mode == 0) {
        src = G.lowest[s];
        val = (float)((double)G.sums[g] / ((double)cnt * 16777216.0));
    } else {
        src = (unsigned)(G.best[r] & 0xFFFFFFFFull);
        int m = G.first_member;                                       // the winner's member: the last one whose base is not above it
        for (int q = G.first_member + 1; q < G.first_member + G.n_members; ++q) if ((unsigned)mem[q].base <= src) m = q;
        const FuseMemberDesc& M = mem[m];
        const long long i = (long long)src - M.base;                  // (0 <= i < M.n: a member of the row's cell)
        if (k < 3) {
            float p[3];
            Src::position(M, T, m, (int)i, p);
            val = move_row(M.pose, k, p[0], p[1], p[2]);              // the winner's MOVED position: the bits insert and gather saw
        } else {
            val = Src::feature(M, T, m, i, k - 3);
        }
    }
    if (k < 3) G.out_xyz[3 * (size_t)r + k] = val; else G.out_feat[5 * (size_t)r + (k - 3)] = val;
    if (k == 0) {
        const u64 mask = G.masks[s];
        if (G.out_count) G.out_count[r] = (int)cnt;
        if (G.out_source) G.out_source[r] = (int)src;
        if (G.out_views) G.out_views[r] = __popcll(mask);
        if (G.out_view_mask) G.out_view_mask[r] = mask;
    }
}

namespace {
// groups, mem: the device's copies of the two tables: every group with points, every member with n > 0 (members of a group consecutive, in order).
// n_max: the largest member n; slots_max, rows_max: the largest slots and rows_cap among the groups.
template <class Src>
hipError_t launch_fuse(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, typename Src::Table T, int n_members, int n_max, int slots_max,
                       int rows_max, float voxel, int mode, int min_points, int min_views, hipStream_t s) {
    if (n_groups <= 0 || n_members <= 0 || n_max <= 0) return hipSuccess;
    const dim3 blk(RB), pts((n_max + RB - 1) / RB, n_members);
    const long long clear = slots_max > 8ll * rows_max ? slots_max : 8ll * rows_max;
    hipLaunchKernelGGL(cvo_fuse_clear_kernel, dim3((unsigned)((clear + RB - 1) / RB), n_groups), blk, 0, s, groups);
    hipLaunchKernelGGL(cvo_fuse_insert_kernel<Src>, pts, blk, 0, s, groups, mem, T, voxel);
    hipLaunchKernelGGL(cvo_fuse_heads_kernel, pts, blk, 0, s, groups, mem, min_points, min_views);
    hipLaunchKernelGGL(cvo_fuse_offsets_kernel, dim3(1, n_groups), blk, 0, s, groups);
    hipLaunchKernelGGL(cvo_fuse_rows_kernel, pts, blk, 0, s, groups, mem, min_points, min_views);
    hipLaunchKernelGGL(cvo_fuse_gather_kernel<Src>, pts, blk, 0, s, groups, mem, T, voxel, mode);
    if (rows_max > 0) hipLaunchKernelGGL(cvo_fuse_write_kernel<Src>, dim3((8 * rows_max + RB - 1) / RB, n_groups), blk, 0, s, groups, mem, T, mode);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_fuse_clouds(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, int n_members, int n_max, int slots_max, int rows_max,
                              float voxel, int mode, int min_points, int min_views, hipStream_t s) {
    return launch_fuse<CloudSource>(groups, n_groups, mem, CloudSource::Table(), n_members, n_max, slots_max, rows_max, voxel, mode, min_points, min_views, s);
}
// the same over frames read in place: frames[q] is the frame of mem[q]
hipError_t launch_fuse_frames(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, const FrameDesc* frames, int n_members, int n, int slots_max,
                              int rows_max, float voxel, int mode, int min_points, int min_views, hipStream_t s) {
    const FrameSource::Table T = {frames};
    return launch_fuse<FrameSource>(groups, n_groups, mem, T, n_members, n, slots_max, rows_max, voxel, mode, min_points, min_views, s);
}
}  // namespace cvohip
