// cvo_map_kernels.hip -- resident maps (NOT in the reference): voxel maps that stay in device memory between calls, to which groups of posed
// clouds or frames are added and from which they are taken away again.  The definition is include/cvo_hip.h's "Resident maps"
// (tests/map_reading.py restates it in numpy); every output is held to it byte for byte.
//
// An update's own cells are a fusion's (cvo_fuse_kernels.hip, the passes clear .. gather as they stand, MEAN, every cell kept): they leave, per
// group, the cells in rank order (row_slot), and per cell its key, member count, member mask and undivided sums.  This file adds what works on
// the maps.  The map is the grid's second dimension everywhere; a MapDesc (cvo_device.h) starts with the MapPlace that says where its rows and
// its table are, and the table's walk, extract's filter, a row's mean and the table's emptying are cvo_voxel_table.hpp's ("a resident map
// read in place"), shared with the views, the probes and the snapshots.
//   an update    lookup   a lane per call-cell: its row in the map (cell_row; -1: absent), the block's births, the refusal bits
//                         (sign -2, "remove what is still there": a cell whose row has none of its members' stamp bits counts as absent
//                         and is skipped, one with some of them is a refusal)
//                offsets  the births' exclusive sums over the blocks and their total (offsets_pass)
//                -- the host waits, refuses or goes on --
//                merge    a lane per call-cell: a born cell takes row rows + (births before it), claims its key's slot by compare-and-swap
//                         and writes its row; an old row's count, mask and stamps are updated.  A call-cell is one lane's and a row is one
//                         call-cell's, so plain stores do
//                sums     a lane per (call-cell, value): the 8 sums added, subtracted or (born) stored: whole cache lines per wave
//   extract      count, offsets, write: a block's 256 rows are ranked by ballot; the 8 values of a row are written by 8 lanes
//   compact      mark, offsets, move (to the rows' other side; it also empties the table), rebuild (a lane per surviving row inserts its key)
//   clear        the table's keys to empty, `live` to 0: of any record that starts with a MapPlace (a refused restore's undo uses it too)
// A merge of maps (cvo_map_merge_kernels.hip) forms its call-cells from a map's rows and then runs lookup .. sums as they stand: what a call-cell
// brings in stamps and mask bits (cell_stamps) is the one thing that differs by source, a template parameter of the merge kernel.
// Integer atomics only (the key's compare-and-swap, a ballot's count added to `live`, an OR of refusal bits); no float atomics; no lane waits
// for another.  Row order never depends on arrival: ranks come from block counts and ballots.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_voxel_table.hpp"

namespace cvohip {
namespace {
constexpr unsigned MAP_MAX_COUNT = 16777215u;                         // CVO_MAP_MAX_COUNT
// the rank of this lane among the block's lanes with `flag`, all 256 threads take part.  The barrier behind the reads lets a kernel call it again
// (the waves' counts are one array per block)
__device__ __forceinline__ int block_rank(bool flag) {
    __shared__ int wave_flags[RB / 64];
    const u64 b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_flags[w] = __popcll(b);
    __syncthreads();
    int r = __popcll(b & ((1ull << lane) - 1ull));
    for (int q = 0; q < w; ++q) r += wave_flags[q];
    __syncthreads();
    return r;
}
// What a call-cell brings besides its key, count and sums -- the bits it sets in view_mask, the least and the largest stamp -- is the one thing
// that differs by where the call-cells come from.  FromMap == false, points (the fuser's passes): the members that touched the cell in slot s
// of its group are its member mask's bits; each gives 1 << (stamp & 63), and lo / hi are the least and the largest of their stamps[].
// FromMap == true, a map's rows (cvo_map_merge_kernels.hip): the slot's mask is the OR of the rows' view_mask as it stands, and the cell of
// rank r keeps in best[r] the largest last_stamp (low word) and, in the high word, the least of ((count >= 1 ? 0 : 2^31) | born): the least born
// among the rows with members, or among all when none has any
template <bool FromMap>
__device__ __forceinline__ u64 cell_stamps(const MapDesc& M, const FuseGroupDesc& G, int s, int r, int* lo, int* hi) {
    if (FromMap) {
        const u64 both = G.best[r];
        *hi = (int)(unsigned)(both & 0xFFFFFFFFull); *lo = (int)((unsigned)(both >> 32) & 0x7FFFFFFFu);
        return G.masks[s];
    }
    u64 bits = 0ull; *lo = 0x7FFFFFFF; *hi = 0;
    for (u64 left = G.masks[s]; left; left &= left - 1ull) {
        const int st = M.stamps[__ffsll((long long)left) - 1];
        bits |= 1ull << (st & 63); *lo = min(*lo, st); *hi = max(*hi, st);
    }
    return bits;
}
// what offsets_pass needs of a record
struct BlockCounts { int* block_heads; int* total; };
// compact's keep rule on row r
__device__ __forceinline__ bool row_stays(const MapDesc& M, int r) {
    if (M.at.count[r] < 1u || M.at.last_stamp[r] < M.filter.min_last_stamp) return false;
    if (__popcll(M.at.mask[r]) < M.filter.min_views && M.at.born[r] < M.probation_from) return false;
    return !M.drop || M.drop[r] == 0;
}
}  // namespace

// ---- an update
__global__ __launch_bounds__(RB) void cvo_map_lookup_kernel(const MapDesc* __restrict__ maps, const FuseGroupDesc* __restrict__ groups) {
    const MapDesc& M = maps[blockIdx.y];
    const FuseGroupDesc& G = groups[M.group];
    const int cells = *G.total, r = blockIdx.x * RB + threadIdx.x;    // (cells <= G.n = rows_cap: every cell has its row_slot and its sums)
    if ((int)blockIdx.x * RB >= cells) return;                        // (uniform over the block)
    bool born = false;
    if (r < cells) {
        const int s = G.row_slot[r];
        const unsigned mem = G.members[s];
        int row = map_lookup(M, G.keys[s]);
        int bad = 0;
        if (M.sign > 0) {
            born = row < 0;                                           // (a group of points has fewer than 2^24 members; a merge's cell may have more)
            if (mem > MAP_MAX_COUNT || (!born && M.at.count[row] + mem > MAP_MAX_COUNT)) bad = 1;   // (then both below 2^24: no wrap)
        } else if (M.sign == -1) {
            if (row < 0) bad = 2; else if (mem > M.at.count[row]) bad = 4;
        } else if (row >= 0) {                                        // -2, remove what is still there: by the row's stamp bits
            int lo, hi;
            const u64 bits = cell_stamps<false>(M, G, s, r, &lo, &hi), have = M.at.mask[row] & bits;   // (only points are removed)
            if (have == 0ull) row = -1;                               // none of these members is in the row: it was dropped and made again
            else if (have != bits) bad = 8;
            else if (mem > M.at.count[row]) bad = 4;
        }
        M.cell_row[r] = row;                                          // (a removal's -1: the cell is skipped)
        if (bad) atomicOr(&M.total[2], bad);
    }
    const int k = __syncthreads_count(born);
    if (threadIdx.x == 0) M.block_heads[blockIdx.x] = k;
}
// which == 0: over the blocks of the map's rows into total[0]; 1: over the blocks of the update's call-cells into total[1]
__global__ __launch_bounds__(RB) void cvo_map_offsets_kernel(const MapDesc* __restrict__ maps, const FuseGroupDesc* __restrict__ groups, int which) {
    const MapDesc& M = maps[blockIdx.y];
    const int n = which ? *groups[M.group].total : M.rows;
    offsets_pass(BlockCounts{M.block_heads, M.total + which}, (n + RB - 1) / RB);
}
template <bool FromMap>
__global__ __launch_bounds__(RB) void cvo_map_merge_kernel(const MapDesc* __restrict__ maps, const FuseGroupDesc* __restrict__ groups) {
    const MapDesc& M = maps[blockIdx.y];
    const FuseGroupDesc& G = groups[M.group];
    const int cells = *G.total, r = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= cells) return;                        // (uniform over the block)
    const bool in = r < cells;
    int row = in ? M.cell_row[r] : 0;
    const bool born = in && row < 0 && M.sign > 0;                    // (a removal has none: its absent cells were refused, or are skipped)
    const int rank = block_rank(born);
    int change = 0;                                                   // of the map's live rows
    if (in && (born || row >= 0)) {
        const int s = G.row_slot[r];
        const unsigned mem = G.members[s];
        int lo, hi;
        const u64 bits = cell_stamps<FromMap>(M, G, s, r, &lo, &hi);  // the members that touched the cell / the rows that went into it
        if (born) {
            row = M.rows + M.block_heads[blockIdx.x] + rank;          // (below max_rows: the host counted the births)
            const u64 key = G.keys[s];
            bool fresh;
            const unsigned t = table_insert(M.tkeys, (unsigned)M.slots, key, &fresh);   // (always fresh: the key is this lane's alone)
            M.trow[t] = row;
            M.at.keys[row] = key; M.at.count[row] = mem; M.at.mask[row] = bits; M.at.last_stamp[row] = hi; M.at.born[row] = lo;
            M.cell_row[r] = -row - 1;
            change = mem >= 1u;                                       // (a merge's cell of dead rows alone is born dead)
        } else if (M.sign > 0) {
            const unsigned c = M.at.count[row];
            M.at.count[row] = c + mem; M.at.mask[row] |= bits; M.at.last_stamp[row] = max(M.at.last_stamp[row], hi);
            if (c == 0u && mem >= 1u) { M.at.born[row] = lo; change = 1; }
        } else {
            const unsigned c = M.at.count[row] - mem;
            M.at.count[row] = c; M.at.mask[row] &= ~bits;
            if (c == 0u) change = -1;
        }
    }
    const int lane = threadIdx.x & 63;
    const int d = __popcll(__ballot(change > 0)) - __popcll(__ballot(change < 0));
    if (lane == 0 && d != 0) atomicAdd(M.live, d);
}
__global__ __launch_bounds__(RB) void cvo_map_sums_kernel(const MapDesc* __restrict__ maps, const FuseGroupDesc* __restrict__ groups) {
    const MapDesc& M = maps[blockIdx.y];
    const FuseGroupDesc& G = groups[M.group];
    const long long g = (long long)blockIdx.x * RB + threadIdx.x;
    if (g >= 8ll * *G.total) return;
    const int v = M.cell_row[g >> 3], k = (int)(g & 7);
    const long long q = G.sums[g];
    if (v < 0) { if (M.sign > 0) M.at.sums[8 * (size_t)(-v - 1) + k] = q; }   // born; a removal's -1 is a skipped cell
    else if (M.sign > 0) M.at.sums[8 * (size_t)v + k] += q;
    else M.at.sums[8 * (size_t)v + k] -= q;
}

// ---- extract
__global__ __launch_bounds__(RB) void cvo_map_xcount_kernel(const MapDesc* __restrict__ maps) {
    const MapDesc& M = maps[blockIdx.y];
    const int r = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.rows) return;                       // (uniform over the block)
    const int k = __syncthreads_count(r < M.rows && row_kept(M.at, M.filter, r));
    if (threadIdx.x == 0) M.block_heads[blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_map_xwrite_kernel(const MapDesc* __restrict__ maps) {
    __shared__ int out_of[RB];
    const MapDesc& M = maps[blockIdx.y];
    const int first = blockIdx.x * RB, r = first + threadIdx.x;
    if (first >= M.rows) return;                                      // (uniform over the block)
    const bool kept = r < M.rows && row_kept(M.at, M.filter, r);
    int o = M.block_heads[blockIdx.x] + block_rank(kept);
    if (!kept || o >= M.cap) o = -1;                                  // rows at or above cap are not written
    out_of[threadIdx.x] = o;
    if (o >= 0) {
        const u64 mask = M.at.mask[r];
        if (M.out_count) M.out_count[o] = (int)M.at.count[r];
        if (M.out_views) M.out_views[o] = __popcll(mask);
        if (M.out_view_mask) M.out_view_mask[o] = mask;
        if (M.out_last_stamp) M.out_last_stamp[o] = M.at.last_stamp[r];
        if (M.out_born) M.out_born[o] = M.at.born[r];
        if (M.out_row) M.out_row[o] = r;
    }
    __syncthreads();
    const int k = threadIdx.x & 7;
    for (int j = 0; j < 8; ++j) {                                     // 32 rows a trip: 8 lanes a row, its 64 bytes of sums
        const int t = j * (RB / 8) + (threadIdx.x >> 3);
        const int at = out_of[t];
        if (at < 0) continue;
        const int row = first + t;
        const float val = row_mean(M.at.sums[8 * (size_t)row + k], M.at.count[row]);
        if (k < 3) M.out_xyz[3 * (size_t)at + k] = val; else M.out_feat[5 * (size_t)at + (k - 3)] = val;
    }
}

// ---- compact
__global__ __launch_bounds__(RB) void cvo_map_mark_kernel(const MapDesc* __restrict__ maps) {
    const MapDesc& M = maps[blockIdx.y];
    const int r = blockIdx.x * RB + threadIdx.x;
    if ((int)blockIdx.x * RB >= M.rows) return;                       // (uniform over the block)
    const int k = __syncthreads_count(r < M.rows && row_stays(M, r));
    if (threadIdx.x == 0) M.block_heads[blockIdx.x] = k;
}
__global__ __launch_bounds__(RB) void cvo_map_move_kernel(const MapDesc* __restrict__ maps) {
    __shared__ int out_of[RB];
    const MapDesc& M = maps[blockIdx.y];
    const int first = blockIdx.x * RB, r = first + threadIdx.x;
    table_empty(M, r, (int)gridDim.x * RB);                           // (nothing reads the table before rebuild, which sets `live`)
    if (first >= M.rows) return;                                      // (uniform over the block)
    const bool stays = r < M.rows && row_stays(M, r);
    const int rank = block_rank(stays);                               // (every thread of the block: it has a barrier)
    const int o = stays ? M.block_heads[blockIdx.x] + rank : -1;
    out_of[threadIdx.x] = o;
    if (r < M.rows && M.new_row) M.new_row[r] = o;
    if (o >= 0) {
        M.to.keys[o] = M.at.keys[r]; M.to.count[o] = M.at.count[r]; M.to.mask[o] = M.at.mask[r];
        M.to.last_stamp[o] = M.at.last_stamp[r]; M.to.born[o] = M.at.born[r];
    }
    __syncthreads();
    const int k = threadIdx.x & 7;
    for (int j = 0; j < 8; ++j) {
        const int t = j * (RB / 8) + (threadIdx.x >> 3);
        const int at = out_of[t];
        if (at >= 0) M.to.sums[8 * (size_t)at + k] = M.at.sums[8 * (size_t)(first + t) + k];
    }
}
// a lane per surviving row (on the side the move wrote): its key into the emptied table
__global__ __launch_bounds__(RB) void cvo_map_rebuild_kernel(const MapDesc* __restrict__ maps) {
    const MapDesc& M = maps[blockIdx.y];
    const int r = blockIdx.x * RB + threadIdx.x, rows = *M.total;
    if (r == 0) *M.live = rows;                                       // (every survivor has count >= 1)
    if (r >= rows) return;
    bool fresh;
    const unsigned t = table_insert(M.tkeys, (unsigned)M.slots, M.to.keys[r], &fresh);
    M.trow[t] = r;
}
// records: MapDescs or MapSnapDescs, `stride` bytes each: the MapPlace a record starts with
__global__ __launch_bounds__(RB) void cvo_map_clear_kernel(const char* __restrict__ records, size_t stride) {
    table_empty(*reinterpret_cast<const MapPlace*>(records + blockIdx.y * stride), blockIdx.x * RB + threadIdx.x, gridDim.x * RB);
}

// maps, groups: the device's copies of the call's tables; n_max: the most call-cells a group can have (its points)
hipError_t launch_map_lookup(const MapDesc* maps, int n_maps, const FuseGroupDesc* groups, int n_max, hipStream_t s) {
    if (n_maps <= 0 || n_max <= 0) return hipSuccess;
    hipLaunchKernelGGL(cvo_map_lookup_kernel, dim3((n_max + RB - 1) / RB, n_maps), dim3(RB), 0, s, maps, groups);
    hipLaunchKernelGGL(cvo_map_offsets_kernel, dim3(1, n_maps), dim3(RB), 0, s, maps, groups, 1);
    return hipGetLastError();
}
// cells_max: the most call-cells of a group, as counted; from_map: the call-cells were formed from maps' rows (cell_stamps)
hipError_t launch_map_merge(const MapDesc* maps, int n_maps, const FuseGroupDesc* groups, int cells_max, bool from_map, hipStream_t s) {
    if (n_maps <= 0 || cells_max <= 0) return hipSuccess;
    const dim3 grid((cells_max + RB - 1) / RB, n_maps);
    if (from_map) hipLaunchKernelGGL(cvo_map_merge_kernel<true>, grid, dim3(RB), 0, s, maps, groups);
    else hipLaunchKernelGGL(cvo_map_merge_kernel<false>, grid, dim3(RB), 0, s, maps, groups);
    hipLaunchKernelGGL(cvo_map_sums_kernel, dim3((unsigned)((8ll * cells_max + RB - 1) / RB), n_maps), dim3(RB), 0, s, maps, groups);
    return hipGetLastError();
}
// rows_max: the most rows among the maps (> 0)
hipError_t launch_map_extract(const MapDesc* maps, int n_maps, int rows_max, bool write, hipStream_t s) {
    const dim3 grid((rows_max + RB - 1) / RB, n_maps);
    hipLaunchKernelGGL(cvo_map_xcount_kernel, grid, dim3(RB), 0, s, maps);
    hipLaunchKernelGGL(cvo_map_offsets_kernel, dim3(1, n_maps), dim3(RB), 0, s, maps, static_cast<const FuseGroupDesc*>(nullptr), 0);
    if (write) hipLaunchKernelGGL(cvo_map_xwrite_kernel, grid, dim3(RB), 0, s, maps);
    return hipGetLastError();
}
hipError_t launch_map_compact(const MapDesc* maps, int n_maps, int rows_max, hipStream_t s) {
    const dim3 grid((rows_max + RB - 1) / RB, n_maps);
    hipLaunchKernelGGL(cvo_map_mark_kernel, grid, dim3(RB), 0, s, maps);
    hipLaunchKernelGGL(cvo_map_offsets_kernel, dim3(1, n_maps), dim3(RB), 0, s, maps, static_cast<const FuseGroupDesc*>(nullptr), 0);
    hipLaunchKernelGGL(cvo_map_move_kernel, grid, dim3(RB), 0, s, maps);
    hipLaunchKernelGGL(cvo_map_rebuild_kernel, grid, dim3(RB), 0, s, maps);
    return hipGetLastError();
}
// records: the device's copy of a table of records that start with a MapPlace, `stride` bytes each; slots: the tables' size
hipError_t launch_map_clear(const void* records, size_t stride, int n_maps, int slots, hipStream_t s) {
    hipLaunchKernelGGL(cvo_map_clear_kernel, dim3((slots + RB - 1) / RB, n_maps), dim3(RB), 0, s, static_cast<const char*>(records), stride);
    return hipGetLastError();
}
}  // namespace cvohip
