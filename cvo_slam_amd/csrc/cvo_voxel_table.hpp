// cvo_voxel_table.hpp -- the device helpers the voxel-grid kernels share (cvo_reduce_kernels.hip, cvo_fuse_kernels.hip): reading a point of a
// cvo_device_cloud or of a frame read in place (the two point sources), its validity and cell key, the open-addressing table's insert, the
// runs of lanes with one cell, -- each written once, over the record type -- the seven passes of a reduction and of a fusion, and the rules of
// a resident map read in place (the map, view, probe and snapshot kernels).  Every one is inlined into its kernel; nothing here has a symbol.
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
// the mean of `count` >= 1 values from the sum of their llrint(v * 2^24): a double product, a double division, one conversion to float -- MEAN's
// write, extract's expression, and what a view and a probe of a map read of a row
__device__ __forceinline__ float row_mean(long long sum, unsigned count) { return (float)((double)sum / ((double)count * 16777216.0)); }

// ---- The passes of a reduction (cvo_reduce_kernels.hip: a record per cloud) and of a fusion (cvo_fuse_kernels.hip: a record per group of posed
// members), each written once over the record type Rec -- ReduceDesc or FuseGroupDesc, which name their table, rows and outputs alike.  A kernel
// finds its record, its point's index g in the record's numbering (a cloud's index; a group's global index, member after member) and its block's
// number among the record's 256-point blocks, loads the (moved) point, and calls its pass.  In stream order, seven launches:
//   clear    the table's keys to empty, lowest to all ones, members to 0; the rows' sums to 0 and bests to all ones
//   insert   a lane per point: validity, key, CAS-insert; atomicMin of g into the slot's `lowest`, atomicAdd into its `members`; the point's slot
//            (-1: invalid) is kept in slot_of for the later passes
//   heads    a block counts its heads: points that are their cell's lowest member in a cell that is kept (at least min_points members)
//   offsets  a block per record turns the blocks' counts into their exclusive sums and writes the record's row count
//   rows     a head's row is its block's offset + the heads before it in the block: rows ascend with the lowest member's g.  The head writes
//            the row into its slot (-1 for the lowest member of a dropped cell), and the slot into row_slot[row] for rows below rows_cap
//   gather   a lane per point again: map[g] = its cell's row; for rows below rows_cap, MEAN adds q = llrint((double)v * 2^24) of its 8 values
//            into the row's 64-bit sums (|v| < 2^15 and n < 2^20: below 2^59), CENTRAL does a 64-bit atomicMin of (d2 bits << 32) | g
//   write    a lane per (row, value): MEAN row_mean of the row's sum and count, CENTRAL the value of the winning member
// Every value that reaches an output is independent of the order in which points arrive: integer atomicAdd / atomicMin / compare-and-swap of a
// key only, no float atomics, and the place of a cell in the table never shows.
// Runs: neighbouring points of a dense cloud mostly share a cell, so in insert and gather a run of consecutive lanes of a wave with one cell acts
// once -- its first lane inserts and gives its g to `lowest`, its last lane adds the run's length to `members`, the run's q (or its least
// (d2, g)) are combined with a segmented scan over __shfl_up and its last lane does the atomics.  Integer sums and minima: the same bits as a
// lane-by-lane form.
// `slot_too(g)` (clear), `kept_too(s)` (head test) and `row_too(r, s)` (write) are where a caller adds what its record has beside these names.

// clear, lane g of the record's grid
template <class Rec, class SlotToo>
__device__ __forceinline__ void clear_pass(const Rec& D, long long g, SlotToo slot_too) {
    if (g < D.slots) { D.keys[g] = KEY_EMPTY; slot_too(g); D.lowest[g] = 0xFFFFFFFFu; D.members[g] = 0u; }
    if (g < 8ll * D.rows_cap) D.sums[g] = 0;
    if (g < D.rows_cap) D.best[g] = KEY_EMPTY;
}
// insert: the slot of point g's cell `key` (KEY_EMPTY: an invalid point, or a lane past the points: no cell, -1).  All 64 lanes of the wave take
// part.  *run_tail: this lane ends a run with a cell -- where a caller does its own once-per-run atomics on the slot.
template <class Rec>
__device__ __forceinline__ int insert_pass(const Rec& D, u64 key, unsigned g, int lane, bool* run_tail) {
    int start; bool tail, fresh;
    lane_runs(key, lane, &start, &tail);
    int s = -1;
    if (key != KEY_EMPTY && lane == start) {                          // a run's first lane holds its lowest index
        s = (int)table_insert(D.keys, (unsigned)D.slots, key, &fresh);
        atomicMin(&D.lowest[s], g);
    }
    s = __shfl(s, start);
    *run_tail = key != KEY_EMPTY && tail;
    if (*run_tail) atomicAdd(&D.members[s], (unsigned)(lane - start + 1));
    return s;
}
// head test: is point g, in slot s (-1: an invalid point, or a lane past the points), the lowest member of a kept cell (1) / of a dropped one
// (2); 0: neither
template <class Rec, class KeptToo>
__device__ __forceinline__ int head_of(const Rec& D, int g, int s, int min_points, KeptToo kept_too) {
    if (s < 0 || D.lowest[s] != (unsigned)g) return 0;
    return D.members[s] >= (unsigned)min_points && kept_too(s) ? 1 : 2;
}
// offsets, one block per record with nb blocks of points: thread t owns `per` consecutive blocks' counts; their sums are scanned through LDS
template <class Rec>
__device__ __forceinline__ void offsets_pass(const Rec& D, int nb) {
    __shared__ int part[RB];
    const int per = (nb + RB - 1) / RB, t = threadIdx.x;
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
// rows, every lane of the record's block number `block`: `what` and s are the lane's head_of
template <class Rec>
__device__ __forceinline__ void rows_pass(const Rec& D, int block, int what, int s) {
    __shared__ int wave_heads[RB / 64];
    const bool head = what == 1, dropped = what == 2;
    const u64 b = __ballot(head);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_heads[w] = __popcll(b);
    __syncthreads();
    if (dropped) D.row[s] = -1;
    if (head) {
        int r = D.block_heads[block] + __popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; ++q) r += wave_heads[q];
        D.row[s] = r;
        if (r < D.rows_cap) D.row_slot[r] = s;
    }
}
// row-of-point: map[g], and the point's row if it is one that is written (-1: none)
template <class Rec>
__device__ __forceinline__ int row_of_point(const Rec& D, bool in, int g) {
    int r = -1;
    if (in) {
        const int s = D.slot_of[g];
        r = s >= 0 ? D.row[s] : -1;
        if (D.out_map) D.out_map[g] = r;
        if (r >= D.rows_cap) r = -1;
    }
    return r;
}
// gather: point g with row r (row_of_point) and the 8 values v that count for it (zeros with r < 0).  All 64 lanes of the wave take part.
template <class Rec>
__device__ __forceinline__ void gather_pass(const Rec& D, int r, const float v[8], unsigned g, int lane, float voxel, int mode) {
    int start; bool tail;
    lane_runs(r, lane, &start, &tail);
    if (mode == 0) {                                                  // CVO_REDUCE_MEAN: a run of lanes with one row adds its q on chip (integers: any order gives the same sum)
        u64 q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = (u64)__double2ll_rn((double)v[k] * 16777216.0);   // (two's complement: the signed sum)
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
    } else {                                                          // CVO_REDUCE_CENTRAL: a run's least (d2 bits, g) the same way
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = floorf(__fdiv_rn(v[k], voxel));
            const float d = __fsub_rn(v[k], __fmul_rn(__fadd_rn(c, 0.5f), voxel));
            d2 = k == 0 ? __fmul_rn(d, d) : __fadd_rn(d2, __fmul_rn(d, d));
        }
        u64 best = r >= 0 ? ((u64)__float_as_uint(d2) << 32) | (u64)g : KEY_EMPTY;
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= start;
            if (__ballot(take) == 0ull) break;
            const u64 up = __shfl_up(best, d);
            if (take && up < best) best = up;
        }
        if (r >= 0 && tail) atomicMin(&D.best[r], best);
    }
}
// write, lane g of the record's grid: value k = g & 7 of row g >> 3.  winner(src, k): value k of member src, CENTRAL's winner -- the caller's,
// which knows where its points are and whether they move
template <class Rec, class Winner, class RowToo>
__device__ __forceinline__ void write_pass(const Rec& D, int g, int mode, Winner winner, RowToo row_too) {
    const int r = g >> 3, k = g & 7;
    if (r >= min(*D.total, D.rows_cap)) return;
    const int s = D.row_slot[r];
    const unsigned cnt = D.members[s];
    unsigned src; float val;
    if (mode == 0) {
        src = D.lowest[s];
        val = row_mean(D.sums[g], cnt);
    } else {
        src = (unsigned)(D.best[r] & 0xFFFFFFFFull);
        val = winner(src, k);
    }
    if (k < 3) D.out_xyz[3 * (size_t)r + k] = val; else D.out_feat[5 * (size_t)r + (k - 3)] = val;
    if (k == 0) {
        if (D.out_count) D.out_count[r] = (int)cnt;
        if (D.out_source) D.out_source[r] = (int)src;
        row_too(r, s);
    }
}

// ---- A resident map read in place (cvo_map_kernels.hip, cvo_view_kernels.hip, cvo_probe_kernels.hip, cvo_map_snapshot_kernels.hip): the rules
// that every kernel over a MapPlace (cvo_device.h) follows bit for bit, each written here once (a row's mean is row_mean, above).
// row r of a moved position: x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3], every product and sum rounded (the fuser's move; the features
// pass through)
__device__ __forceinline__ float move_row(const float* M, int r, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(M[4 * r], x), __fadd_rn(__fmul_rn(M[4 * r + 1], y), __fmul_rn(M[4 * r + 2], z))), M[4 * r + 3]);
}
// the row of `key` in the map, -1: absent.  The table is at most half full, and a slot's key never changes between two rebuilds.
__device__ __forceinline__ int map_lookup(const MapPlace& P, u64 key) {
    unsigned s = home_slot(key, (unsigned)P.slots);
    for (;;) {
        const u64 k = P.tkeys[s];
        if (k == key) return P.trow[s];
        if (k == KEY_EMPTY) return -1;
        s = s + 1 == (unsigned)P.slots ? 0u : s + 1;
    }
}
// extract's filter on row r of R: a kept row has count >= 1
__device__ __forceinline__ bool row_kept(const MapRows& R, const MapRowFilter& F, int r) {
    const unsigned c = R.count[r];
    return c >= (unsigned)max(1, F.min_points) && __popcll(R.mask[r]) >= F.min_views && R.last_stamp[r] >= F.min_last_stamp;
}
// the table's keys to empty and `live` to 0, lane g of a grid of `lanes` lanes over the map (slots, and a grid sized for them or for the rows, are
// below 2^22)
__device__ __forceinline__ void table_empty(const MapPlace& P, int g, int lanes) {
    if (g == 0) *P.live = 0;
    for (; g < P.slots; g += lanes) P.tkeys[g] = KEY_EMPTY;
}
}  // namespace
}  // namespace cvohip
