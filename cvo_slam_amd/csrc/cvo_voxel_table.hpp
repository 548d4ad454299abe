// cvo_voxel_table.hpp -- the device helpers the voxel-grid kernels share (cvo_reduce_kernels.hip, cvo_fuse_kernels.hip): reading a point of a
// cvo_device_cloud or of a frame read in place (the two point sources), its validity and cell key, the open-addressing table's insert, and the
// runs of lanes with one cell.  Every one is inlined into its kernel; nothing here has a symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"

namespace cvohip {
namespace {
typedef unsigned long long u64;
constexpr u64 KEY_EMPTY = ~0ull;
constexpr int RB = 256;   // block size of every voxel-grid kernel

// point i's 8 floats: position, then the 5 features (i < n: inside the checked extents)
__device__ __forceinline__ void load_point(const float* xyz, const float* feat, long long xs, long long ps, long long cs, int i, float v[8]) {
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(xyz) + (long long)i * xs);
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    const char* f = reinterpret_cast<const char*>(feat) + (long long)i * ps;
#pragma unroll
    for (int c = 0; c < 5; ++c) v[3 + c] = *reinterpret_cast<const float*>(f + c * cs);
}
// ---- Where a kernel's points come from: the template parameter of the passes that read points (insert, gather, CENTRAL's write, count-insert).
// A source gives point i of record D (a ReduceDesc, CountDesc or FuseMemberDesc) as a position and 5 features; `which` is the record's place in
// the source's table.  bounded_features: the features are valid by construction, so a point's validity and cell need its position alone.
struct CloudSource {                                                  // a cvo_device_cloud: the arrays are the record's own, no table
    struct Table {};
    static constexpr bool bounded_features = false;
    template <class Rec> static __device__ __forceinline__ void position(const Rec& D, Table, int, int i, float p[3]) {
        const float* q = reinterpret_cast<const float*>(reinterpret_cast<const char*>(D.xyz) + (long long)i * D.xyz_stride);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    template <class Rec> static __device__ __forceinline__ float feature(const Rec& D, Table, int, long long i, int c) {
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(D.feat) + i * D.feat_point_stride + c * D.feat_channel_stride);
    }
    template <class Rec> static __device__ __forceinline__ void point(const Rec& D, Table, int, int i, float v[8]) {
        load_point(D.xyz, D.feat, D.xyz_stride, D.feat_point_stride, D.feat_channel_stride, i, v);
    }
};
// An RGB-D frame read in place (cvo_hip.h, "Reducing frames"): point i is a sub-grid pixel, its position the generator's float sequence on the
// pixel's depth (pcd_cloud_kernel), its features the pixel's B, G, R and the generator's level-0 gradients on the FLAT index (pcd_gray_kernel,
// pcd_grad_kernel), computed from the colour bytes of the pixel and its four flat neighbours.  A block's 256 points are consecutive sub-grid
// pixels, so the neighbours' bytes are cache hits.  Nothing outside the image's rows is read: the gradient's neighbours exist for rows
// 1 .. h - 2 only, and there (x - 1, y) at x == 0 is (w - 1, y - 1), (x + 1, y) at x == w - 1 is (0, y + 1).
struct FrameSource {
    struct Table { const FrameDesc* frames; };
    static constexpr bool bounded_features = true;                    // bytes, and half differences of bytes
    static __device__ __forceinline__ void pixel(const FrameDesc& F, int i, int* x, int* y) {
        const int r = i / F.ws;
        *x = (i - r * F.ws) * F.step; *y = r * F.step;
    }
    static __device__ __forceinline__ const uint8_t* colour(const FrameDesc& F, int x, int y) { return F.bgr + (long long)y * F.bgr_pitch + x * F.pixel_bytes; }
    static __device__ __forceinline__ float gray(const FrameDesc& F, int x, int y) {
        const uint8_t* c = colour(F, x, y);
        const int b = c[F.swap_rb ? 2 : 0], g = c[1], r = c[F.swap_rb ? 0 : 2];
        return (float)((b * 4899 + g * 9617 + r * 1868 + (1 << 13)) >> 14);
    }
    static __device__ __forceinline__ float grad_x(const FrameDesc& F, int x, int y) {
        if (y < 1 || y > F.h - 2) return 0.f;
        const float right = x + 1 < F.w ? gray(F, x + 1, y) : gray(F, 0, y + 1), left = x > 0 ? gray(F, x - 1, y) : gray(F, F.w - 1, y - 1);
        return __fmul_rn(0.5f, __fsub_rn(right, left));
    }
    static __device__ __forceinline__ float grad_y(const FrameDesc& F, int x, int y) {
        if (y < 1 || y > F.h - 2) return 0.f;
        return __fmul_rn(0.5f, __fsub_rn(gray(F, x, y + 1), gray(F, x, y - 1)));
    }
    static __device__ __forceinline__ void position_at(const FrameDesc& F, int x, int y, float p[3]) {
        const unsigned d = *reinterpret_cast<const uint16_t*>(F.depth + (long long)y * F.depth_pitch + 2 * x);
        const float z = __fdiv_rn((float)d, F.scaling_factor);
        p[0] = __fdiv_rn(__fmul_rn(__fsub_rn((float)x, F.cx), z), F.fx);
        p[1] = __fdiv_rn(__fmul_rn(__fsub_rn((float)y, F.cy), z), F.fy);
        p[2] = z;
        if (d == 0u) p[0] = p[1] = p[2] = __uint_as_float(0x7FC00000u);   // no depth: invalid by the reducer's own rule
    }
    template <class Rec> static __device__ __forceinline__ void position(const Rec&, Table T, int which, int i, float p[3]) {
        const FrameDesc& F = T.frames[which];
        int x, y; pixel(F, i, &x, &y);
        position_at(F, x, y, p);
    }
    template <class Rec> static __device__ __forceinline__ float feature(const Rec&, Table T, int which, long long i, int c) {
        const FrameDesc& F = T.frames[which];
        int x, y; pixel(F, (int)i, &x, &y);
        if (c == 3) return grad_x(F, x, y);
        if (c == 4) return grad_y(F, x, y);
        return (float)colour(F, x, y)[c == 1 ? 1 : (c == 0) != (F.swap_rb != 0) ? 0 : 2];
    }
    template <class Rec> static __device__ __forceinline__ void point(const Rec&, Table T, int which, int i, float v[8]) {
        const FrameDesc& F = T.frames[which];
        int x, y; pixel(F, i, &x, &y);
        position_at(F, x, y, v);
        const uint8_t* c = colour(F, x, y);
        v[3] = (float)c[F.swap_rb ? 2 : 0]; v[4] = (float)c[1]; v[5] = (float)c[F.swap_rb ? 0 : 2];
        v[6] = grad_x(F, x, y); v[7] = grad_y(F, x, y);
    }
};
// the floats a point's validity and cell need: all 8, or the position alone before features that cannot be invalid
template <class Src, class Rec>
__device__ __forceinline__ void point_for_cell(const Rec& D, typename Src::Table T, int which, int i, float v[8]) {
    if (Src::bounded_features) {
        Src::position(D, T, which, i, v);
#pragma unroll
        for (int k = 3; k < 8; ++k) v[k] = 0.f;
    } else {
        Src::point(D, T, which, i, v);
    }
}
// validity and cell: all 8 floats finite and below 2^15 (NaN and inf compare false), |floorf(x / voxel)| < 2^20
__device__ __forceinline__ bool cell_of(const float v[8], float voxel, float c[3], u64* key) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok &= fabsf(v[k]) < 32768.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = floorf(__fdiv_rn(v[k], voxel)); ok &= fabsf(c[k]) < 1048576.f; }
    if (!ok) return false;
    *key = ((u64)(unsigned)((int)c[0] + 1048576) << 42) | ((u64)(unsigned)((int)c[1] + 1048576) << 21) | (u64)(unsigned)((int)c[2] + 1048576);
    return true;
}
__device__ __forceinline__ unsigned home_slot(u64 h, unsigned slots) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return (unsigned)(((h >> 32) * (u64)slots) >> 32);
}
// The slot of `key`, claimed if no point has claimed one yet (*fresh: by this lane).  A slot's key changes once, from empty to its cell's, so a
// relaxed device-scope load that shows a key is final; only an empty slot is worth the compare-and-swap.  No lane waits for another.
__device__ __forceinline__ unsigned table_insert(u64* keys, unsigned slots, u64 key, bool* fresh) {
    unsigned s = home_slot(key, slots);
    *fresh = false;
    for (;;) {
        u64 k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == KEY_EMPTY) {
            k = atomicCAS(&keys[s], KEY_EMPTY, key);
            if (k == KEY_EMPTY) { *fresh = true; return s; }
        }
        if (k == key) return s;
        s = s + 1 == slots ? 0u : s + 1;
    }
}
// Runs of consecutive lanes with the same id (all 64 lanes of the wave take part): the lane at which this lane's run starts, and whether it ends
// here.  Neighbouring points of a dense cloud mostly share a cell, so a run does its cell's atomics once (Guideline 12: sum on chip first).
template <class Id>
__device__ __forceinline__ void lane_runs(Id id, int lane, int* start, bool* tail) {
    const Id prev = __shfl_up(id, 1);
    const u64 heads = __ballot(lane == 0 || prev != id);
    *start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    *tail = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0ull;
}
}  // namespace
}  // namespace cvohip
