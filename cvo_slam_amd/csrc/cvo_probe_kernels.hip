// cvo_probe_kernels.hip -- probing resident maps with posed clouds and frames (NOT in the reference): for every point of a member under a pose,
// the map row it falls into or lies nearest to.  The definition is include/cvo_hip.h's "Probing maps" (tests/map_probe_reading.py restates it
// in numpy); every output is held to it byte for byte.
//
// All probes of a call go through the same two launches, the PROBE in the grid's second dimension: all lanes of a block belong to one probe,
// read one pose and one map (uniform loads) and never search for their probe.
//   probe    a lane per point: move, validity and cell by the fuser's rules (move_row, cell_of); the walk of the map's table (map_lookup) for
//            the point's own cell (reach 0) or for the 27 cells around it (reach 1); extract's filter on the rows found (row_kept); the squared
//            distance to a kept row's mean position (row_mean); the least (d2 bits, row) wins -- each rule cvo_voxel_table.hpp's.  The lane writes
//            its point's outputs and a byte of 1 into `hit` at its row; the block stores its four class counts
//   sum      a block per probe adds the blocks' counts up and stores the probe's four
// The points come from the kernel's template parameter, as in the reducer: a cvo_device_cloud (CloudSource) or an RGB-D frame read in place
// (FrameSource, probe q's frame at frames[q]).  A lane reads 24 of a row's 64 bytes of sums, and count, mask and last_stamp, and only of rows
// that the table holds.  The maps are read only.  No atomics at all: a point's outputs are its lane's, every writer of a hit byte stores the
// same 1 (the call clears the bytes on the stream first), and the counts go through per-block stores and the sum kernel, as the views'
// relation counts do.  No lane waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
constexpr int ROW_ABSENT = -1, ROW_INVALID = -3, ROW_FILTERED = -4;
constexpr int ROW_NO_POINT = -2;                                      // a lane past the member's points: in no class
// the squared distance of the moved position w to the mean position of kept row r (count >= 1): every product and sum rounded
__device__ __forceinline__ float probe_dist2(const MapRows& R, int r, const float w[3]) {
    const long long* q = R.sums + 8 * (size_t)r;
    const unsigned c = R.count[r];
    const float dx = __fsub_rn(w[0], row_mean(q[0], c)), dy = __fsub_rn(w[1], row_mean(q[1], c)), dz = __fsub_rn(w[2], row_mean(q[2], c));
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
}  // namespace

template <class Src>
__global__ __launch_bounds__(RB) void cvo_probe_kernel(const ProbeDesc* __restrict__ probes, typename Src::Table T, float voxel) {
    __shared__ int wave_class[RB / 64][4];
    const ProbeDesc& P = probes[blockIdx.y];
    const MapRows& R = P.map.at;
    const int i = blockIdx.x * RB + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)blockIdx.x * RB >= P.n) return;                          // (uniform over the block; past that every lane stays for the ballots)
    int row = ROW_NO_POINT;
    float d2 = __uint_as_float(0x7F800000u);
    if (i < P.n) {
        float v[8], w[8], c[3];
        u64 key;
        point_for_cell<Src>(P, T, blockIdx.y, i, v);
#pragma unroll
        for (int r = 0; r < 3; ++r) w[r] = move_row(P.pose, r, v[0], v[1], v[2]);
#pragma unroll
        for (int k = 3; k < 8; ++k) w[k] = v[k];
        const bool src_ok = fabsf(v[0]) < 32768.f && fabsf(v[1]) < 32768.f && fabsf(v[2]) < 32768.f;   // (the features are w's)
        if (!cell_of(w, voxel, c, &key) || !src_ok) {
            row = ROW_INVALID;
        } else if (P.reach == 0) {
            const int r = map_lookup(P.map, key);
            if (r < 0) row = ROW_ABSENT;
            else if (!row_kept(R, P.filter, r)) row = ROW_FILTERED;
            else { row = r; d2 = probe_dist2(R, r, w); }
        } else {
            const int cx = (int)c[0], cy = (int)c[1], cz = (int)c[2];
            u64 best = KEY_EMPTY;                                     // the least (d2 bits << 32) | row: d2 >= 0, so the bits order as the floats do
            bool any = false;
            for (int j = 0; j < 27; ++j) {
                const int nx = cx + j / 9 - 1, ny = cy + (j / 3) % 3 - 1, nz = cz + j % 3 - 1;
                if (abs(nx) >= 1048576 || abs(ny) >= 1048576 || abs(nz) >= 1048576) continue;   // in no map: its key is never formed
                const u64 k = ((u64)(unsigned)(nx + 1048576) << 42) | ((u64)(unsigned)(ny + 1048576) << 21) | (u64)(unsigned)(nz + 1048576);
                const int r = map_lookup(P.map, k);
                if (r < 0) continue;
                any = true;
                if (!row_kept(R, P.filter, r)) continue;
                const u64 cand = ((u64)__float_as_uint(probe_dist2(R, r, w)) << 32) | (u64)(unsigned)r;
                if (cand < best) best = cand;
            }
            if (best != KEY_EMPTY) { row = (int)(unsigned)(best & 0xFFFFFFFFull); d2 = __uint_as_float((unsigned)(best >> 32)); }
            else row = any ? ROW_FILTERED : ROW_ABSENT;
        }
        if (P.out_row) P.out_row[i] = row;
        if (P.out_dist2) P.out_dist2[i] = d2;                         // (0x7F800000 where row < 0)
        if (P.out_count) P.out_count[i] = row >= 0 ? (int)R.count[row] : 0;
        if (P.out_views) P.out_views[i] = row >= 0 ? __popcll(R.mask[row]) : 0;
        if (P.out_last_stamp) P.out_last_stamp[i] = row >= 0 ? R.last_stamp[row] : 0;
        if (P.out_hit && row >= 0) P.out_hit[row] = 1;                // (row < rows: the table's own; every writer stores the same byte)
    }
    // the block's four counts: found, absent, filtered, invalid
    const int cls = row >= 0 ? 0 : row == ROW_ABSENT ? 1 : row == ROW_FILTERED ? 2 : row == ROW_INVALID ? 3 : -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = __popcll(__ballot(cls == q));
        if (lane == 0) wave_class[wv][q] = k;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int k = 0;
        for (int q = 0; q < RB / 64; ++q) k += wave_class[q][threadIdx.x];
        P.block_counts[4 * (size_t)blockIdx.x + threadIdx.x] = k;
    }
}
__global__ __launch_bounds__(RB) void cvo_probe_sum_kernel(const ProbeDesc* __restrict__ probes) {
    __shared__ int wave_sum[RB / 64][4];
    const ProbeDesc& P = probes[blockIdx.y];
    const int nb = (P.n + RB - 1) / RB, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int k[4] = {0, 0, 0, 0};
    for (int j = threadIdx.x; j < nb; j += RB) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] += P.block_counts[4 * (size_t)j + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int d = 32; d > 0; d >>= 1) k[q] += __shfl_down(k[q], d);
        if (lane == 0) wave_sum[wv][q] = k[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int t = 0;
        for (int q = 0; q < RB / 64; ++q) t += wave_sum[q][threadIdx.x];
        P.totals[threadIdx.x] = t;
    }
}

namespace {
// probes: the device's copy of the call's table, one record per probe, empty members included (their four counts are 0); n_max: the largest n
template <class Src>
hipError_t launch_probe(const ProbeDesc* probes, typename Src::Table T, int n_probes, int n_max, float voxel, hipStream_t s) {
    if (n_probes <= 0) return hipSuccess;
    if (n_max > 0) hipLaunchKernelGGL(cvo_probe_kernel<Src>, dim3((n_max + RB - 1) / RB, n_probes), dim3(RB), 0, s, probes, T, voxel);
    hipLaunchKernelGGL(cvo_probe_sum_kernel, dim3(1, n_probes), dim3(RB), 0, s, probes);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_probe_clouds(const ProbeDesc* probes, int n_probes, int n_max, float voxel, hipStream_t s) {
    return launch_probe<CloudSource>(probes, CloudSource::Table(), n_probes, n_max, voxel, s);
}
// the same over frames read in place: frames[q] is the frame of probes[q]
hipError_t launch_probe_frames(const ProbeDesc* probes, const FrameDesc* frames, int n_probes, int n, float voxel, hipStream_t s) {
    const FrameSource::Table T = {frames};
    return launch_probe<FrameSource>(probes, T, n_probes, n, voxel, s);
}
}  // namespace cvohip
