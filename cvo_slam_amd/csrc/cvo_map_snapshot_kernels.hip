// cvo_map_snapshot_kernels.hip -- saving and restoring resident maps (NOT in the reference): a map's rows copied out as they stand, and a map
// made of rows that the caller gives.  The definition is include/cvo_hip.h's "Saving and restoring maps" (tests/map_snapshot_reading.py restates
// it in numpy); every byte is held to it.  The map is the grid's second dimension everywhere; a MapSnapDesc (cvo_device.h) starts with the
// MapPlace that says where the map's rows and its table are, and adds the caller's arrays.
//   snapshot   copy     a lane per row: key, count, mask and the two stamps; a row's 64 bytes of sums by 8 lanes.  Rows 0 .. rows - 1, dead ones
//                       included; nothing behind them
//   restore    write    the caller's rows are untrusted.  A lane per row reads its fields ONCE, tests them (key, count, stamps), and writes them
//                       to the side the map is not on; 8 lanes a row do the same with the sums, against the count the block has just read.  The
//                       refusal bits are OR-ed into the call's figures.  The launch also empties the table and zeroes `live` (table_empty, as move does)
//              insert   a lane per row inserts the key it reads from the map's OWN copy (a bad key is not inserted): a lane that is not `fresh`
//                       has met its key's twin -- the duplicate bit.  A ballot's count of the rows with count >= 1 is added to `live`
//              -- the host waits; on success it flips the side and sets rows; on a refusal, for EVERY listed map: --
//              clear    cvo_map_kernels.hip's, over these records: the table's keys to empty, `live` to 0
//              insert   the same kernel over the rows the map still has on its old side, dead ones included, `live` counted again
// Integer atomics only (the key's compare-and-swap, a ballot's count added to `live`, an OR of refusal bits); no lane waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
constexpr unsigned SNAP_MAX_COUNT = 16777215u;                        // CVO_MAP_MAX_COUNT
constexpr u64 SNAP_SUM_BOUND = (1ull << 39) - (1ull << 15);           // a member's largest |llrint(v * 2^24)| ("Viewing maps")
// bit 63 clear and each of the three 21-bit fields in 1 .. 2^21 - 1 (all ones, the table's empty mark, has bit 63)
__device__ __forceinline__ bool key_valid(u64 key) {
    return (key >> 63) == 0ull && ((key >> 42) & 0x1FFFFFull) != 0ull && ((key >> 21) & 0x1FFFFFull) != 0ull && (key & 0x1FFFFFull) != 0ull;
}
// |sum| <= count * (2^39 - 2^15), exactly: from count 2^25 on the bound is above 2^63 and holds for every int64
__device__ __forceinline__ bool sum_in_bound(long long sum, unsigned count) {
    if (count >= (1u << 25)) return true;
    const u64 a = sum < 0 ? 0ull - (u64)sum : (u64)sum;
    return a <= (u64)count * SNAP_SUM_BOUND;
}
}  // namespace

__global__ __launch_bounds__(RB) void cvo_map_snapshot_kernel(const MapSnapDesc* __restrict__ maps) {
    const MapSnapDesc& M = maps[blockIdx.y];
    const int first = blockIdx.x * RB, r = first + threadIdx.x;
    if (first >= M.rows) return;                                      // (uniform over the block)
    if (r < M.rows) {
        M.ext.keys[r] = M.at.keys[r]; M.ext.count[r] = M.at.count[r]; M.ext.mask[r] = M.at.mask[r];
        M.ext.last_stamp[r] = M.at.last_stamp[r]; M.ext.born[r] = M.at.born[r];
    }
    const long long end = 8ll * M.rows;
    for (int j = 0; j < 8; ++j) {                                     // 32 rows a trip: 8 lanes a row, its 64 bytes of sums
        const long long g = 8ll * first + j * RB + threadIdx.x;
        if (g < end) M.ext.sums[g] = M.at.sums[g];
    }
}

__global__ __launch_bounds__(RB) void cvo_map_restore_write_kernel(const MapSnapDesc* __restrict__ maps) {
    __shared__ unsigned count_of[RB];
    const MapSnapDesc& M = maps[blockIdx.y];
    const int first = blockIdx.x * RB, r = first + threadIdx.x;
    table_empty(M, r, (int)gridDim.x * RB);                           // (nothing reads the table before insert)
    if (first >= M.ext_rows) return;                                  // (uniform over the block)
    int bad = 0;
    unsigned c = 0u;
    if (r < M.ext_rows) {
        const u64 key = M.ext.keys[r], mask = M.ext.mask[r];
        const int last = M.ext.last_stamp[r], born = M.ext.born[r];
        c = M.ext.count[r];
        if (!key_valid(key)) bad |= 1;
        if (c > SNAP_MAX_COUNT) bad |= 2;
        if (last < 0 || born < 0) bad |= 4;
        M.to.keys[r] = key; M.to.count[r] = c; M.to.mask[r] = mask; M.to.last_stamp[r] = last; M.to.born[r] = born;
    }
    count_of[threadIdx.x] = c;
    __syncthreads();
    const long long end = 8ll * M.ext_rows;
    for (int j = 0; j < 8; ++j) {
        const int t = j * (RB / 8) + (threadIdx.x >> 3);              // the block's row of this lane in trip j
        const long long g = 8ll * first + j * RB + threadIdx.x;
        if (g < end) {
            const long long q = M.ext.sums[g];
            if (!sum_in_bound(q, count_of[t])) bad |= 8;
            M.to.sums[g] = q;
        }
    }
    if (bad) atomicOr(&M.figures[1], bad);
}
// old == 0: the rows a restore has just written (`to`, ext_rows of them), with the duplicate test; old == 1: the rows the map has (`at`, rows)
__global__ __launch_bounds__(RB) void cvo_map_restore_insert_kernel(const MapSnapDesc* __restrict__ maps, int old) {
    const MapSnapDesc& M = maps[blockIdx.y];
    const MapRows& R = old ? M.at : M.to;
    const int n = old ? M.rows : M.ext_rows, r = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= n) return;                            // (uniform over the block)
    bool alive = false;
    if (r < n) {
        const u64 key = R.keys[r];
        alive = R.count[r] >= 1u;
        if (key_valid(key)) {                                         // (a bad key is refused already; all ones must never reach the table)
            bool fresh;
            const unsigned t = table_insert(M.tkeys, (unsigned)M.slots, key, &fresh);
            if (fresh) M.trow[t] = r; else atomicOr(&M.figures[1], 16);
        }
    }
    const int k = __popcll(__ballot(alive));
    if ((threadIdx.x & 63) == 0 && k != 0) atomicAdd(M.live, k);
}

hipError_t launch_map_clear(const void* records, size_t stride, int n_maps, int slots, hipStream_t s);   // cvo_map_kernels.hip
// maps: the device's copy of the call's table; rows_max: the most rows among the maps (> 0)
hipError_t launch_map_snapshot(const MapSnapDesc* maps, int n_maps, int rows_max, hipStream_t s) {
    hipLaunchKernelGGL(cvo_map_snapshot_kernel, dim3((rows_max + RB - 1) / RB, n_maps), dim3(RB), 0, s, maps);
    return hipGetLastError();
}
// rows_max: the most rows to put in among the maps (may be 0: the tables are emptied all the same)
hipError_t launch_map_restore(const MapSnapDesc* maps, int n_maps, int rows_max, hipStream_t s) {
    const dim3 grid((std::max(rows_max, 1) + RB - 1) / RB, n_maps);
    hipLaunchKernelGGL(cvo_map_restore_write_kernel, grid, dim3(RB), 0, s, maps);
    if (rows_max > 0) hipLaunchKernelGGL(cvo_map_restore_insert_kernel, grid, dim3(RB), 0, s, maps, 0);
    return hipGetLastError();
}
// a refused restore: every listed map's table again from the rows it has; rows_max: the most such rows (may be 0), slots: the table's size
hipError_t launch_map_restore_undo(const MapSnapDesc* maps, int n_maps, int rows_max, int slots, hipStream_t s) {
    const hipError_t e = launch_map_clear(maps, sizeof(MapSnapDesc), n_maps, slots, s);
    if (e != hipSuccess) return e;
    if (rows_max > 0) hipLaunchKernelGGL(cvo_map_restore_insert_kernel, dim3((rows_max + RB - 1) / RB, n_maps), dim3(RB), 0, s, maps, 1);
    return hipGetLastError();
}
}  // namespace cvohip
