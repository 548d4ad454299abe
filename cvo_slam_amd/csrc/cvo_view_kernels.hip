// cvo_view_kernels.hip -- viewing posed device clouds, and resident maps where they lie, from a camera (NOT in the reference): the z-buffered
// visible subset of the points and the z-buffer itself.  The definitions are include/cvo_hip.h's "Viewing clouds" and "Viewing maps"
// (tests/view_reading.py and tests/map_view_reading.py restate them in numpy); every output is held to them byte for byte.
//
// All views of a call go through the same launches, the VIEW in the grid's second dimension: all lanes of a block belong to one view, read one
// pose and one camera (uniform loads) and never search for their view.  Six launches, seven with observed depth, whatever the number of views:
//   clear    the z-cells to all ones, the four relation counts to 0
//   project  a lane per point: move, validity, range, project; its z-cell number (or -2: valid but not in view, -3: invalid, -4: a map's row
//            that its filter drops) is kept in `code`;
//            an in-view point does ONE 64-bit atomicMin of (z' bits << 32) | index into its z-cell
//   count    a lane per point: is it visible?  FRONT: its z-cell's key carries its index.  SURFACE: the slack test against the front's bits.  A
//            block stores __syncthreads_count of its visible lanes
//   offsets  offsets_pass of cvo_voxel_table.hpp as it is: a block per view turns the blocks' counts into exclusive sums and the row count
//   write    a lane per point: its row is its block's offset + the visible lanes before it in the block (ballot and popcount, as rows_pass);
//            map; for rows below cap the moved position, the features, source, pixel and relation; with observed depth a block stores the four
//            relation counts of its rows, those at or above cap too, and a map's carve byte is stored per row
//   relation a block per view adds the blocks' relation counts up (only with observed depth)
//   images   a lane per z-cell: depth and index (only when a view asked for one of them)
// The points come from the passes' template parameter, as in the reducer: a cvo_device_cloud (ViewCloudSource: "Viewing clouds"), or the rows
// of a resident map where they lie (ViewMapSource: "Viewing maps"; a MapViewSrc per view behind the ViewDesc records).  A map's row is a
// point when its filter keeps it (row_kept; code -4 otherwise: never divided, projected or counted); its floats are extract's expression on the
// row's sums and count (row_mean), its index the row number; the rules are cvo_voxel_table.hpp's, as the move is (move_row).  project, count and write read points and are instantiated per source; clear, offsets, relation
// and images read the z-buffer, the codes and the counts alone and are shared.  A lane takes a row: the visible rows, whose 64 bytes of sums
// are read whole, are a small share of a map, and project and count read a row's 24 bytes of position sums.
// z' is never stored: count and write compute it again by the same __fmul_rn / __fadd_rn sequence (move_z), as the fuser recomputes moved
// positions; for a map that is three f64 divisions more per in-view row in SURFACE mode alone (FRONT compares indices), which does not show
// in a call's time (profiles/map_views.txt: SURFACE is not slower than FRONT), and keeps a view's region at 4 bytes per row.
// Integer atomics only: a 64-bit atomicMin per in-view point, integer atomicAdd for the relation counts.  The blocks of a view do not add
// into the view's four counters themselves: 4800 waves' atomics on one cache line took 3 ms of a 4.5 ms call (64 views of 307200 points);
// they store their counts, and one block per view sums them and does 16 atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
constexpr int CODE_OUTSIDE = -2, CODE_INVALID = -3, CODE_FILTERED = -4;
// ---- Where a view's points come from: `which` is the view's place in the call (its ViewDesc and, for a map, its MapViewSrc).
struct ViewCloudSource {                                              // a cvo_device_cloud: the arrays are the record's own, no table
    struct Table {};
    static constexpr bool bounded_features = false;
    static __device__ __forceinline__ bool takes_part(const ViewDesc&, Table, int, int) { return true; }
    static __device__ __forceinline__ void position(const ViewDesc& V, Table, int, int i, float p[3]) {
        const float* q = reinterpret_cast<const float*>(reinterpret_cast<const char*>(V.xyz) + (long long)i * V.xyz_stride);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    static __device__ __forceinline__ void point(const ViewDesc& V, Table, int, int i, float v[8]) {
        load_point(V.xyz, V.feat, V.xyz_stride, V.feat_point_stride, V.feat_channel_stride, i, v);
    }
    static __device__ __forceinline__ void carve(Table, int, int, bool) {}
};
// A resident map's rows read in place: row i is a point when the view's filter keeps it (row_kept, so count >= 1), and then its floats are
// row_mean's.  bounded_features: the feature means are means of floats below 2^15 in every supported map state (cvo_hip.h, "Viewing
// maps"), so validity needs the position alone: 24 of a row's 64 bytes of sums.
struct ViewMapSource {
    struct Table { const MapViewSrc* maps; };
    static constexpr bool bounded_features = true;
    static __device__ __forceinline__ bool takes_part(const ViewDesc&, Table T, int which, int i) {
        const MapViewSrc& S = T.maps[which];
        return row_kept(S.map.at, S.filter, i);
    }
    static __device__ __forceinline__ void position(const ViewDesc&, Table T, int which, int i, float p[3]) {
        const MapViewSrc& S = T.maps[which];
        const long long* q = S.map.at.sums + 8 * (size_t)i;
        const unsigned c = S.map.at.count[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = row_mean(q[k], c);
    }
    static __device__ __forceinline__ void point(const ViewDesc&, Table T, int which, int i, float v[8]) {
        const MapViewSrc& S = T.maps[which];
        const long long* q = S.map.at.sums + 8 * (size_t)i;
        const unsigned c = S.map.at.count[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row_mean(q[k], c);
    }
    static __device__ __forceinline__ void carve(Table T, int which, int i, bool seen_through) {
        uint8_t* out = T.maps[which].carve;
        if (out) out[i] = seen_through ? 1 : 0;
    }
};
// point i's z' alone (i < n, a point that takes part)
template <class Src>
__device__ __forceinline__ float move_z(const ViewDesc& V, typename Src::Table T, int which, int i) {
    float p[3];
    Src::position(V, T, which, i, p);
    return move_row(V.pose, 2, p[0], p[1], p[2]);
}
// the pixel of a moved position w, if it is in view
__device__ __forceinline__ bool project(const ViewDesc& V, const ViewParams& P, const float w[3], int* px, int* py) {
    if (!(P.z_near <= w[2] && w[2] <= P.z_far)) return false;
    const float u = __fadd_rn(__fdiv_rn(__fmul_rn(w[0], V.fx), w[2]), V.cx), v = __fadd_rn(__fdiv_rn(__fmul_rn(w[1], V.fy), w[2]), V.cy);
    if (!(fabsf(u) < 1048576.f && fabsf(v) < 1048576.f)) return false;   // (NaN and inf compare false)
    *px = (int)floorf(__fadd_rn(u, 0.5f)); *py = (int)floorf(__fadd_rn(v, 0.5f));
    return *px >= 0 && *px < P.width && *py >= 0 && *py < P.height;
}
// is point i, with z-cell number c >= 0, visible?
template <class Src>
__device__ __forceinline__ bool visible(const ViewDesc& V, typename Src::Table T, int which, const ViewParams& P, int i, int c) {
    const u64 front = V.zbuf[c];
    if (P.mode == 0) return (unsigned)(front & 0xFFFFFFFFull) == (unsigned)i;
    const float zf = __uint_as_float((unsigned)(front >> 32));
    return move_z<Src>(V, T, which, i) <= __fadd_rn(zf, __fmul_rn(P.slack, zf));
}
}  // namespace

__global__ __launch_bounds__(RB) void cvo_view_clear_kernel(const ViewDesc* __restrict__ views, ViewParams P) {
    const ViewDesc& V = views[blockIdx.y];
    const int g = blockIdx.x * RB + threadIdx.x;
    if (g < P.gw * P.gh) V.zbuf[g] = KEY_EMPTY;
    if (g < 4) V.relation_counts[g] = 0;
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_view_project_kernel(const ViewDesc* __restrict__ views, typename Src::Table T, ViewParams P) {
    const ViewDesc& V = views[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= V.n) return;
    int c = CODE_FILTERED, px, py;
    if (Src::takes_part(V, T, blockIdx.y, i)) {
        float v[8], w[3];
        if (Src::bounded_features) {                                  // (the features cannot be invalid: the position alone is read)
            Src::position(V, T, blockIdx.y, i, v);
#pragma unroll
            for (int k = 3; k < 8; ++k) v[k] = 0.f;
        } else {
            Src::point(V, T, blockIdx.y, i, v);
        }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) ok &= fabsf(v[k]) < 32768.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) { w[r] = move_row(V.pose, r, v[0], v[1], v[2]); ok &= fabsf(w[r]) < 32768.f; }
        c = CODE_INVALID;
        if (ok) {
            c = CODE_OUTSIDE;
            if (project(V, P, w, &px, &py)) {
                c = (py / P.cell) * P.gw + px / P.cell;
                atomicMin(&V.zbuf[c], ((u64)__float_as_uint(w[2]) << 32) | (u64)(unsigned)i);
            }
        }
    }
    V.code[i] = c;
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_view_count_kernel(const ViewDesc* __restrict__ views, typename Src::Table T, ViewParams P) {
    const ViewDesc& V = views[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= V.n) return;                          // (uniform over the block)
    const int c = i < V.n ? V.code[i] : CODE_INVALID;
    const int k = __syncthreads_count(c >= 0 && visible<Src>(V, T, blockIdx.y, P, i, c));
    if (threadIdx.x == 0) V.block_heads[blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_view_offsets_kernel(const ViewDesc* __restrict__ views) {
    const ViewDesc& V = views[blockIdx.y];
    offsets_pass(V, (V.n + RB - 1) / RB);
}
template <class Src>
__global__ __launch_bounds__(RB) void cvo_view_write_kernel(const ViewDesc* __restrict__ views, typename Src::Table T, ViewParams P) {
    __shared__ int wave_rows[RB / 64];
    const ViewDesc& V = views[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)blockIdx.x * RB >= V.n) return;                          // (uniform over the block; past that every lane stays for the ballots)
    const int c = i < V.n ? V.code[i] : CODE_INVALID;
    const bool vis = c >= 0 && visible<Src>(V, T, blockIdx.y, P, i, c);
    const u64 b = __ballot(vis);
    if (lane == 0) wave_rows[wv] = __popcll(b);
    __syncthreads();
    int row = -1, rel = -1;
    if (vis) {
        row = V.block_heads[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < wv; ++q) row += wave_rows[q];
        float v[8], w[3];
        Src::point(V, T, blockIdx.y, i, v);
#pragma unroll
        for (int r = 0; r < 3; ++r) w[r] = move_row(V.pose, r, v[0], v[1], v[2]);
        int px = 0, py = 0;
        project(V, P, w, &px, &py);                                   // (in view: project said so for these bits)
        if (V.observed) {
            const unsigned d = *reinterpret_cast<const uint16_t*>(V.observed + (long long)py * V.observed_pitch + 2 * px);
            const float zo = __fdiv_rn((float)d, V.scaling_factor), t = __fmul_rn(P.depth_tol, zo);
            rel = d == 0u ? 0 : w[2] < __fsub_rn(zo, t) ? 1 : w[2] > __fadd_rn(zo, t) ? 3 : 2;
        }
        if (row < V.cap) {
            float* x = V.out_xyz + 3 * (size_t)row; float* f = V.out_feat + 5 * (size_t)row;
            x[0] = w[0]; x[1] = w[1]; x[2] = w[2];
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = v[3 + k];
            if (V.out_source) V.out_source[row] = i;
            if (V.out_pixel) V.out_pixel[row] = py * P.width + px;
            if (V.out_relation && rel >= 0) V.out_relation[row] = rel;
        }
    }
    if (i < V.n && V.out_map) V.out_map[i] = vis ? row : c >= 0 ? -1 : c;
    if (i < V.n) Src::carve(T, blockIdx.y, i, rel == 1);              // (a map's carve byte: the camera saw through this visible row, whatever cap is)
    if (V.observed) {                                                 // (uniform over the block) the block's four counts
        __shared__ int wave_rel[RB / 64][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = __popcll(__ballot(rel == q));
            if (lane == 0) wave_rel[wv][q] = k;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            int k = 0;
            for (int q = 0; q < RB / 64; ++q) k += wave_rel[q][threadIdx.x];
            V.block_relations[4 * (size_t)blockIdx.x + threadIdx.x] = k;
        }
    }
}
__global__ __launch_bounds__(RB) void cvo_view_relation_kernel(const ViewDesc* __restrict__ views) {
    const ViewDesc& V = views[blockIdx.y];
    if (!V.observed) return;
    const int nb = (V.n + RB - 1) / RB, lane = threadIdx.x & 63;
    int k[4] = {0, 0, 0, 0};
    for (int j = threadIdx.x; j < nb; j += RB) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] += V.block_relations[4 * (size_t)j + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int d = 32; d > 0; d >>= 1) k[q] += __shfl_down(k[q], d);
        if (lane == 0 && k[q] > 0) atomicAdd(&V.relation_counts[q], k[q]);
    }
}
__global__ __launch_bounds__(RB) void cvo_view_images_kernel(const ViewDesc* __restrict__ views, ViewParams P) {
    const ViewDesc& V = views[blockIdx.y];
    const int g = blockIdx.x * RB + threadIdx.x;
    if (g >= P.gw * P.gh) return;
    const u64 front = V.zbuf[g];
    if (V.out_depth) V.out_depth[g] = front == KEY_EMPTY ? 0.f : __uint_as_float((unsigned)(front >> 32));
    if (V.out_index) V.out_index[g] = front == KEY_EMPTY ? -1 : (int)(unsigned)(front & 0xFFFFFFFFull);
}

namespace {
// views: the device's copy of the call's table, one record per view, empty clouds included; n_max: the largest n; observed: the call has
// observed depth; images: a view asked for depth or index
template <class Src>
hipError_t launch_view(const ViewDesc* views, typename Src::Table T, int n_views, int n_max, const ViewParams& P, bool observed, bool images, hipStream_t s) {
    if (n_views <= 0) return hipSuccess;
    const dim3 blk(RB), cells((P.gw * P.gh + RB - 1) / RB, n_views), pts((n_max + RB - 1) / RB, n_views);
    hipLaunchKernelGGL(cvo_view_clear_kernel, cells, blk, 0, s, views, P);
    if (n_max > 0) {
        hipLaunchKernelGGL(cvo_view_project_kernel<Src>, pts, blk, 0, s, views, T, P);
        hipLaunchKernelGGL(cvo_view_count_kernel<Src>, pts, blk, 0, s, views, T, P);
    }
    hipLaunchKernelGGL(cvo_view_offsets_kernel, dim3(1, n_views), blk, 0, s, views);
    if (n_max > 0) hipLaunchKernelGGL(cvo_view_write_kernel<Src>, pts, blk, 0, s, views, T, P);
    if (n_max > 0 && observed) hipLaunchKernelGGL(cvo_view_relation_kernel, dim3(1, n_views), blk, 0, s, views);
    if (images) hipLaunchKernelGGL(cvo_view_images_kernel, cells, blk, 0, s, views, P);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_view_clouds(const ViewDesc* views, int n_views, int n_max, const ViewParams& P, bool observed, bool images, hipStream_t s) {
    return launch_view<ViewCloudSource>(views, ViewCloudSource::Table(), n_views, n_max, P, observed, images, s);
}
// the same over maps read in place: maps[q] is the map of views[q], whose n is the map's rows (dead ones included) and whose cloud fields are 0
hipError_t launch_view_maps(const ViewDesc* views, const MapViewSrc* maps, int n_views, int n_max, const ViewParams& P, bool observed, bool images, hipStream_t s) {
    const ViewMapSource::Table T = {maps};
    return launch_view<ViewMapSource>(views, T, n_views, n_max, P, observed, images, s);
}
}  // namespace cvohip
