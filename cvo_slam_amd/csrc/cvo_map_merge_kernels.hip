// cvo_map_merge_kernels.hip -- merging resident maps (NOT in the reference): the kept rows of a source map added into a destination map of the
// same voxel or of one 2^level times as large.  The definition is include/cvo_hip.h's "Merging maps" (tests/map_merge_reading.py restates it on
// map_reading.Map); every byte of the destination is held to it.
//
// Cells nest: the cell of a point at voxel * 2^level is its cell at `voxel` with each coordinate shifted right by level, arithmetically, so a
// coarse cell's sums, count and mask are the integer sum, sum and OR of its children's.  This file is a merge's FIRST half: it forms the
// merge's call-cells from a MapPlace's rows in the group's region of the reducer's scratch, where an update's fusion passes form theirs from
// points, and leaves what an update's second half expects -- *total, row_slot, and per cell its key, its count (members) and its eight sums by
// rank -- and, in place of member masks and stamps[], per cell the OR of the rows' view_mask (masks) and the stamps by rank (best, the layout
// cell_stamps<true> of cvo_map_kernels.hip reads).  The second half -- lookup, offsets, the host's wait, merge, sums -- is the update's own.
// The merge is the grid's second dimension everywhere; six launches whatever the number of merges:
//   clear    the group's table, sums and stamps (clear_pass; best's all ones is "no stamp yet" for both words)
//   insert   a lane per source row: the keep test (all rows, or extract's row_kept), the shifted key, table_insert; atomicMin of the row number
//            into the slot's `lowest`, the row's count added to `members`, its view_mask OR-ed into `masks`; the row's slot is kept in slot_of
//   heads, offsets, rows   the fuser's ranking (head_of, offsets_pass, rows_pass): call-cells ascend with their lowest source row number
//   gather   a lane per (source row, value): the row's sum added to its cell's, by rank; lane 0 of a row gives its stamps to the cell's
// A cell's count is a 32-bit sum of up to 4096 counts below 2^24 and could wrap out of sight: the lane whose add carries out of 32 bits (the
// addends are non-negative, so the true sum is at least 2^32 exactly when some add carries) sets the destination's count refusal bit itself;
// a sum that did not wrap and is above 16777215 is lookup's to refuse.
// Integer atomics only (the key's compare-and-swap, atomicMin of the lowest row, 32-bit and 64-bit adds, OR, max, min); no float atomics; no
// lane waits for another.  Row order comes from ranks, never from arrival order.  The source is only read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
// a cell key with each of its three 21-bit fields f replaced by ((f - 2^20) >> level) + 2^20: the cell at a voxel 2^level times as large
__device__ __forceinline__ u64 shifted_key(u64 key, int level) {
    u64 out = 0ull;
#pragma unroll
    for (int sh = 42; sh >= 0; sh -= 21) {
        const int c = (int)((key >> sh) & 0x1FFFFFull) - 1048576;     // (a signed cell coordinate: >> is arithmetic)
        out |= (u64)(unsigned)((c >> level) + 1048576) << sh;
    }
    return out;
}
struct EveryCell { __device__ __forceinline__ bool operator()(int) const { return true; } };
}  // namespace

__global__ __launch_bounds__(RB) void cvo_map_cells_clear_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const FuseGroupDesc& G = groups[merges[blockIdx.y].group];
    clear_pass(G, (long long)blockIdx.x * RB + threadIdx.x, [&](long long g) { G.masks[g] = 0ull; });
}
__global__ __launch_bounds__(RB) void cvo_map_cells_insert_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const MapMergeDesc& D = merges[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= D.rows) return;                                          // (D.rows == G.n <= the region's points: slot_of has room)
    const FuseGroupDesc& G = groups[D.group];
    int s = -1;
    if (D.all_rows || row_kept(D.at, D.filter, i)) {
        bool fresh;
        s = (int)table_insert(G.keys, (unsigned)G.slots, shifted_key(D.at.keys[i], D.level), &fresh);
        atomicMin(&G.lowest[s], (unsigned)i);
        const unsigned c = D.at.count[i];
        if (c != 0u && atomicAdd(&G.members[s], c) > ~c) atomicOr(&D.figures[2], 1);   // (old + c carries: the cell's count is 2^32 or more)
        const u64 mask = D.at.mask[i];
        if (mask != 0ull) atomicOr(&G.masks[s], mask);
    }
    G.slot_of[i] = s;
}
__global__ __launch_bounds__(RB) void cvo_map_cells_heads_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const MapMergeDesc& D = merges[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.rows) return;                       // (uniform over the block)
    const FuseGroupDesc& G = groups[D.group];
    const int s = i < D.rows ? G.slot_of[i] : -1;
    const int k = __syncthreads_count(head_of(G, i, s, 0, EveryCell()) == 1);   // (a cell of dead rows alone has 0 members and is kept)
    if (threadIdx.x == 0) G.block_heads[blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_map_cells_offsets_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const FuseGroupDesc& G = groups[merges[blockIdx.y].group];
    offsets_pass(G, G.n_blocks);
}
__global__ __launch_bounds__(RB) void cvo_map_cells_rows_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const MapMergeDesc& D = merges[blockIdx.y];
    const int i = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= D.rows) return;                       // (uniform over the block)
    const FuseGroupDesc& G = groups[D.group];
    const int s = i < D.rows ? G.slot_of[i] : -1;
    rows_pass(G, blockIdx.x, head_of(G, i, s, 0, EveryCell()), s);
}
__global__ __launch_bounds__(RB) void cvo_map_cells_gather_kernel(const MapMergeDesc* __restrict__ merges, const FuseGroupDesc* __restrict__ groups) {
    const MapMergeDesc& D = merges[blockIdx.y];
    const long long g = (long long)blockIdx.x * RB + threadIdx.x;     // value g & 7 of source row g >> 3: a wave reads 8 rows' 512 bytes of sums
    if (g >= 8ll * D.rows) return;
    const FuseGroupDesc& G = groups[D.group];
    const int i = (int)(g >> 3), k = (int)(g & 7);
    const int s = G.slot_of[i];
    if (s < 0) return;                                                // the row is not kept
    const int r = G.row[s];                                           // (below rows_cap == the source's rows: a cell has at least one of them)
    const long long q = D.at.sums[g];
    if (q != 0) atomicAdd(reinterpret_cast<u64*>(G.sums) + 8 * (size_t)r + k, (u64)q);   // (two's complement: the signed sum)
    if (k == 0) {
        unsigned* words = reinterpret_cast<unsigned*>(G.best + r);    // low word: the largest last_stamp; high word: cell_stamps' packed least born
        atomicMax(reinterpret_cast<int*>(words), D.at.last_stamp[i]); // (from -1, all ones: stamps are >= 0)
        atomicMin(words + 1, (D.at.count[i] >= 1u ? 0u : 0x80000000u) | (unsigned)D.at.born[i]);
    }
}

// merges, groups: the device's copies of the call's two tables, a group per merge; rows_max: the most source rows among the merges (> 0)
hipError_t launch_map_merge_cells(const MapMergeDesc* merges, int n_merges, const FuseGroupDesc* groups, int rows_max, hipStream_t s) {
    if (n_merges <= 0 || rows_max <= 0) return hipSuccess;
    const dim3 blk(RB), rows((rows_max + RB - 1) / RB, n_merges);
    hipLaunchKernelGGL(cvo_map_cells_clear_kernel, dim3((unsigned)((8ll * rows_max + RB - 1) / RB), n_merges), blk, 0, s, merges, groups);   // (8 sums a row; 2 slots)
    hipLaunchKernelGGL(cvo_map_cells_insert_kernel, rows, blk, 0, s, merges, groups);
    hipLaunchKernelGGL(cvo_map_cells_heads_kernel, rows, blk, 0, s, merges, groups);
    hipLaunchKernelGGL(cvo_map_cells_offsets_kernel, dim3(1, n_merges), blk, 0, s, merges, groups);
    hipLaunchKernelGGL(cvo_map_cells_rows_kernel, rows, blk, 0, s, merges, groups);
    hipLaunchKernelGGL(cvo_map_cells_gather_kernel, dim3((unsigned)((8ll * rows_max + RB - 1) / RB), n_merges), blk, 0, s, merges, groups);
    return hipGetLastError();
}
}  // namespace cvohip
