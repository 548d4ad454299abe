// cvo_voxel_table.hpp -- the device helpers the voxel-grid kernels share (cvo_reduce_kernels.hip, cvo_fuse_kernels.hip): reading a point of a
// cvo_device_cloud, its validity and cell key, the open-addressing table's insert, and the runs of lanes with one cell.  Every one is inlined
// into its kernel; nothing here has a symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
