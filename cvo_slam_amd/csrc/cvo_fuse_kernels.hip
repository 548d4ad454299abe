// cvo_fuse_kernels.hip -- fusing posed device clouds into voxel-reduced local maps (NOT in the reference): the seven passes of a reduction
// (cvo_voxel_table.hpp) over a GROUP of clouds, each under its pose.  The definition is include/cvo_hip.h's "Fusing clouds"
// (tests/fuse_reading.py restates it in numpy): a fusion is the reduction of the concatenation of the moved members, plus the views filter and
// the two view outputs; every output is held to it bit for bit.  This file adds the members, the move, and the view masks.
//
// The group's points have global indices: member after member.  A group has ONE table (slots = 2 x its points) and one set of rows; the passes
// over points have the MEMBER in the grid's second dimension, so all lanes of a block belong to one member, read one pose (uniform loads) and
// never search for their member.  A member's 256-point blocks have consecutive block numbers in its group (first_block + blockIdx.x), members in
// order: the heads / offsets / rows passes rank by global index exactly as a reduction ranks by index.  Seven launches, whatever the numbers of
// groups and members.
//
// A point's moved position is x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3] by __fmul_rn / __fadd_rn: no contraction, the same bits wherever it
// is computed again (move_row of cvo_voxel_table.hpp: insert, gather, and the CENTRAL write of the winner).  Valid: the 8 source floats and the 3 moved ones finite and below
// 2^15, the cell coordinates of the moved position below 2^20.
//
// View masks: a cell's mask is the OR of 1 << member number over its members -- cleared with the table, set by insert once per run of lanes
// with one cell (an integer atomic, as the passes' own), a term of the head test (a kept cell has at least min_views set bits), and written
// as views and view_mask beside count and source.
// insert, gather and write take the point source as a template parameter (cvo_voxel_table.hpp): a member is a cvo_device_cloud (CloudSource) or
// an RGB-D frame read in place (FrameSource, member q's frame at frames[q]; cvo_fuse_device_frames).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
// member point i (i < n): its source floats v, and w = (moved position, features); for_cell: what validity and cell need (point_for_cell)
template <class Src>
__device__ __forceinline__ void load_moved(const FuseMemberDesc& M, typename Src::Table T, int which, int i, bool for_cell, float v[8], float w[8]) {
    if (for_cell) point_for_cell<Src>(M, T, which, i, v); else Src::point(M, T, which, i, v);
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = move_row(M.pose, r, v[0], v[1], v[2]);
#pragma unroll
    for (int k = 3; k < 8; ++k) w[k] = v[k];
}
// the head test's views term
struct EnoughViews {
    const FuseGroupDesc& G; int min_views;
    __device__ __forceinline__ bool operator()(int s) const { return __popcll(G.masks[s]) >= min_views; }
};
}  // namespace

__global__ __launch_bounds__(RB) void cvo_fuse_clear_kernel(const FuseGroupDesc* __restrict__ groups) {
    const FuseGroupDesc& G = groups[blockIdx.y];
    clear_pass(G, (long long)blockIdx.x * RB + threadIdx.x, [&](long long g) { G.masks[g] = 0ull; });
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
    bool run_tail;
    const int s = insert_pass(G, key, (unsigned)(M.base + i), lane, &run_tail);
    if (run_tail) atomicOr(&G.masks[s], 1ull << M.bit);
    if (i < M.n) G.slot_of[M.base + i] = s;
}
__global__ __launch_bounds__(RB) void cvo_fuse_heads_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, int min_points, int min_views) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block)
    const FuseGroupDesc& G = groups[M.group];
    const int s = i < M.n ? G.slot_of[M.base + i] : -1;
    const int k = __syncthreads_count(head_of(G, M.base + i, s, min_points, EnoughViews{G, min_views}) == 1);
    if (threadIdx.x == 0) G.block_heads[M.first_block + blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_fuse_offsets_kernel(const FuseGroupDesc* __restrict__ groups) {
    const FuseGroupDesc& G = groups[blockIdx.y];
    offsets_pass(G, G.n_blocks);
}
__global__ __launch_bounds__(RB) void cvo_fuse_rows_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, int min_points, int min_views) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block)
    const FuseGroupDesc& G = groups[M.group];
    const int s = i < M.n ? G.slot_of[M.base + i] : -1;
    rows_pass(G, M.first_block + blockIdx.x, head_of(G, M.base + i, s, min_points, EnoughViews{G, min_views}), s);
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_fuse_gather_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, typename Src::Table T,
                                                             float voxel, int mode) {
    const FuseMemberDesc& M = mem[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63;
    if ((int)blockIdx.x * RB >= M.n) return;                          // (uniform over the block; past that every lane stays for the shuffles)
    const FuseGroupDesc& G = groups[M.group];
    const int r = row_of_point(G, i < M.n, M.base + i);
    float v[8], w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 0) load_moved<Src>(M, T, blockIdx.y, i, false, v, w);
    gather_pass(G, r, w, (unsigned)(M.base + i), lane, voxel, mode);
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_fuse_write_kernel(const FuseGroupDesc* __restrict__ groups, const FuseMemberDesc* __restrict__ mem, typename Src::Table T,
                                                            int mode) {
    const FuseGroupDesc& G = groups[blockIdx.y];
    write_pass(G, blockIdx.x * RB + threadIdx.x, mode, [&](unsigned src, int k) {
        int m = G.first_member;                                       // the winner's member: the last one whose base is not above it
        for (int q = G.first_member + 1; q < G.first_member + G.n_members; ++q) if ((unsigned)mem[q].base <= src) m = q;
        const FuseMemberDesc& M = mem[m];
        const long long i = (long long)src - M.base;                  // (0 <= i < M.n: a member of the row's cell)
        if (k >= 3) return Src::feature(M, T, m, i, k - 3);
        float p[3];
        Src::position(M, T, m, (int)i, p);
        return move_row(M.pose, k, p[0], p[1], p[2]);                 // the winner's MOVED position: the bits insert and gather saw
    }, [&](int r, int s) {
        const u64 mask = G.masks[s];
        if (G.out_views) G.out_views[r] = __popcll(mask);
        if (G.out_view_mask) G.out_view_mask[r] = mask;
    });
}

namespace {
// groups, mem: the device's copies of the two tables: every group with points, every member with n > 0 (members of a group consecutive, in order).
// n_max: the largest member n; slots_max, rows_max: the largest slots and rows_cap among the groups.  write == false: the passes clear .. gather
// alone -- the groups' cells with their undivided sums stay in the scratch for the caller's own passes (cvo_map_kernels.hip).
template <class Src>
hipError_t launch_fuse(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, typename Src::Table T, int n_members, int n_max, int slots_max,
                       int rows_max, float voxel, int mode, int min_points, int min_views, hipStream_t s, bool write = true) {
    if (n_groups <= 0 || n_members <= 0 || n_max <= 0) return hipSuccess;
    const dim3 blk(RB), pts((n_max + RB - 1) / RB, n_members);
    const long long clear = slots_max > 8ll * rows_max ? slots_max : 8ll * rows_max;
    hipLaunchKernelGGL(cvo_fuse_clear_kernel, dim3((unsigned)((clear + RB - 1) / RB), n_groups), blk, 0, s, groups);
    hipLaunchKernelGGL(cvo_fuse_insert_kernel<Src>, pts, blk, 0, s, groups, mem, T, voxel);
    hipLaunchKernelGGL(cvo_fuse_heads_kernel, pts, blk, 0, s, groups, mem, min_points, min_views);
    hipLaunchKernelGGL(cvo_fuse_offsets_kernel, dim3(1, n_groups), blk, 0, s, groups);
    hipLaunchKernelGGL(cvo_fuse_rows_kernel, pts, blk, 0, s, groups, mem, min_points, min_views);
    hipLaunchKernelGGL(cvo_fuse_gather_kernel<Src>, pts, blk, 0, s, groups, mem, T, voxel, mode);
    if (rows_max > 0 && write) hipLaunchKernelGGL(cvo_fuse_write_kernel<Src>, dim3((8 * rows_max + RB - 1) / RB, n_groups), blk, 0, s, groups, mem, T, mode);
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
// a fusion's cells without its write: MEAN, every cell kept (min_points = min_views = 1); frames == nullptr: the members are clouds
hipError_t launch_fuse_cells(const FuseGroupDesc* groups, int n_groups, const FuseMemberDesc* mem, const FrameDesc* frames, int n_members, int n_max, int slots_max,
                             int rows_max, float voxel, hipStream_t s) {
    const FrameSource::Table T = {frames};
    return frames ? launch_fuse<FrameSource>(groups, n_groups, mem, T, n_members, n_max, slots_max, rows_max, voxel, 0, 1, 1, s, false)
                  : launch_fuse<CloudSource>(groups, n_groups, mem, CloudSource::Table(), n_members, n_max, slots_max, rows_max, voxel, 0, 1, 1, s, false);
}
}  // namespace cvohip
