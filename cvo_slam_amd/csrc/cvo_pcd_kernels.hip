// cvo_pcd_kernels.hip -- the point-cloud generator in front of the alignment
// (SURVEY.md 8f next-1): what cvo::set_pcd (cvo.cpp:345-386) runs on an RGB-D frame.
//   gray image            cv::cvtColor(COLOR_RGB2GRAY) on the BGR bytes, pcd_generator.cpp:624
//   3-level pyramid       make_pyramid, pcd_generator.cpp:50-143
//   block thresholds      PixelSelector::makeHists, PixelSelector2.cpp:71-134
//   hierarchical select   PixelSelector::select, PixelSelector2.cpp:286-433
//   sub-sampling          PixelSelector::makeMaps, PixelSelector2.cpp:252-268
//   cloud                 get_points_from_pixels + get_features(type 1), pcd_generator.cpp:456-499, 590-612
// Image-sized, memory-bound work: every kernel is one pass over w*h (or fewer) elements with
// coalesced accesses; the selection has no cross-block dependence (the reference's random
// direction table is read but unused, setting_selectDirectionDistribution = false), so 16
// lanes share one 4pot x 4pot block.  The cloud is written straight into the two float4
// planes the alignment kernels read: no host round trip for the points.
// Batches of images (cvo_batch_set_pairs_images): every kernel takes the image as blockIdx.y, each image's buffers lying at a fixed
// stride behind the first one's (the single-frame path is image 0 of a grid one image high); makeMaps' decisions run on the device
// (pcd_decide_kernel, and the sub-sampling kernel derives its own threshold), so a batch is a fixed list of launches and one host sync.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "cvo_device.h"

namespace cvohip {

// ---- load_image: 8-bit gray, OpenCV's fixed-point weights on the first/second/third byte (pcd_generator.cpp:624)
__global__ void pcd_gray_kernel(const uint8_t* __restrict__ bgr, float* __restrict__ I0, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bgr += 3 * (size_t)n * blockIdx.y; I0 += (size_t)n * blockIdx.y;
    const int c0 = bgr[3 * (size_t)i], c1 = bgr[3 * (size_t)i + 1], c2 = bgr[3 * (size_t)i + 2];
    I0[i] = (float)((c0 * 4899 + c1 * 9617 + c2 * 1868 + (1 << 13)) >> 14);
}

// ---- make_pyramid: 2x2 box down-sampling (pcd_generator.cpp:103-118)
// (pn: elements of the parent level's plane, the stride of its images)
// The parent's rows are stepped by the reference's prev_wl = wl*2 (:103), not by the parent's width: the same for an even parent width; for
// an odd one the parent is read sheared, a pixel further per row pair -- what the reference computes.  The last element read is
// 2wl * 2hl - 1, inside the parent plane (2wl <= its width, 2hl <= its height).
__global__ void pcd_down_kernel(const float* __restrict__ P, int pn, float* __restrict__ I, int wl, int hl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= wl * hl) return;
    P += (size_t)pn * blockIdx.y; I += (size_t)wl * hl * blockIdx.y;
    const int x = i % wl, y = i / wl, pw = 2 * wl;
    const float* p = P + (size_t)2 * x + (size_t)2 * y * pw;
    I[i] = 0.25f * (p[0] + p[1] + p[pw] + p[pw + 1]);
}

// ---- make_pyramid: central differences over the FLAT index range [wl, wl*(hl-1)) (pcd_generator.cpp:122-136):
// the first and last column use the neighbouring row's pixel, exactly like the reference
__global__ void pcd_grad_kernel(const float* __restrict__ I, int wl, int hl, float* __restrict__ dx_out, float* __restrict__ dy_out,
                                float* __restrict__ abs2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= wl * hl) return;
    const size_t o = (size_t)wl * hl * blockIdx.y;
    I += o; abs2 += o;
    float dx = 0.f, dy = 0.f, a = 0.f;
    if (idx >= wl && idx < wl * (hl - 1)) {
        dx = 0.5f * (I[idx + 1] - I[idx - 1]);
        dy = 0.5f * (I[idx + wl] - I[idx - wl]);
        if (!__builtin_isfinite(dx)) dx = 0.f;
        if (!__builtin_isfinite(dy)) dy = 0.f;
        a = dx * dx + dy * dy;
    }
    if (dx_out) { dx_out[o + idx] = dx; dy_out[o + idx] = dy; }
    abs2[idx] = a;
}

// ---- makeHists: one workgroup per 32x32 block: histogram of int(sqrt(|grad|^2)) capped at 48, median + 7 (PixelSelector2.cpp:83-103)
__global__ __launch_bounds__(256) void pcd_hist_kernel(const float* __restrict__ abs0, int w, int h, int w32, float* __restrict__ ths) {
    __shared__ int hist[100];
    const int tid = threadIdx.x, bx = blockIdx.x % w32, by = blockIdx.x / w32;
    abs0 += (size_t)w * h * blockIdx.y; ths += (size_t)(w32 * (h / 32) + 100) * blockIdx.y;   // (+100: the zeroed slack, pcd_smooth_kernel)
    if (tid < 100) hist[tid] = 0;
    __syncthreads();
    for (int k = tid; k < 1024; k += 256) {
        const int it = (k & 31) + 32 * bx, jt = (k >> 5) + 32 * by;
        if (it > w - 2 || jt > h - 2 || it < 1 || jt < 1) continue;
        int g = (int)sqrtf(abs0[(size_t)it + (size_t)jt * w]);
        if (g > 48) g = 48;
        atomicAdd(&hist[g + 1], 1); atomicAdd(&hist[0], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int th = (int)(hist[0] * 0.5f + 0.5f), q = 90;               // computeHistQuantil(hist, setting_minGradHistCut), :59-68
        for (int i = 0; i < 90; ++i) { th -= hist[i + 1]; if (th < 0) { q = i; break; } }
        ths[blockIdx.x] = (float)(q + 7);                             // + setting_minGradHistAdd
    }
}

// ---- makeHists: squared 3x3 box mean of the block thresholds (PixelSelector2.cpp:105-132; sums of small integers: exact in any order)
__global__ void pcd_smooth_kernel(const float* __restrict__ ths, int w32, int h32, float* __restrict__ ths_smoothed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w32 * h32) return;
    ths += (size_t)(w32 * h32 + 100) * blockIdx.y; ths_smoothed += (size_t)(w32 * h32 + 100) * blockIdx.y;
    const int x = i % w32, y = i / w32;
    float sum = 0.f, num = 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || xx >= w32 || yy < 0 || yy >= h32) continue;
            num += 1.f; sum += ths[xx + yy * w32];
        }
    ths_smoothed[i] = (sum / num) * (sum / num);
}

// ---- select (PixelSelector2.cpp:286-433).  16 lanes share one 4pot x 4pot block, one lane per pot x pot cell, cells numbered
// in the reference's traversal order (2pot block by 2pot block).  With setting_selectDirectionDistribution = false the walk
// reduces to three order-free rules, each a "first maximum in traversal order":
//   a cell picks its largest |grad|^2 above the level-0 threshold (map = 1);
//   a 2pot block none of whose pixels passes level 0 picks its largest level-1 value above the level-1 threshold (map = 2);
//   a 4pot block none of whose pixels passes level 0 or level 1 picks its largest level-2 value above its threshold (map = 4).
// (In the reference a level-0 hit sets bestIdx3 = bestIdx4 = -2 for good and a level-1 hit sets bestIdx4 = -2 for good: whatever
// was found at the coarser levels before is dropped, and nothing is looked for after.)
// map: 0 / 1 / 2 / 4 per pixel (pre-zeroed); counts[0..2] += n2, n3, n4.
// Batches: image blockIdx.y counts at counts + cstride * image; pot_img (not null: the re-selection pass) gives each image's potential at the
// same stride, 0 = the image keeps its first selection, and the grid is sized for the smallest potential -- workgroups past an image's blocks leave.
__global__ __launch_bounds__(256) void pcd_select_kernel(const float* __restrict__ abs0, const float* __restrict__ abs1, const float* __restrict__ abs2,
                                                         const float* __restrict__ ths_smoothed, int w, int h, int pot, const int* __restrict__ pot_img,
                                                         uint8_t* __restrict__ map, int* __restrict__ counts, int cstride) {
    const int img = blockIdx.y;
    if (pot_img) { pot = pot_img[(size_t)cstride * img]; if (pot <= 0) return; }
    const int nbx = (w + 4 * pot - 1) / (4 * pot), nby = (h + 4 * pot - 1) / (4 * pot);
    if ((int)((blockIdx.x * blockDim.x) >> 4) >= nbx * nby) return;    // (uniform: the whole workgroup)
    abs0 += (size_t)w * h * img; abs1 += (size_t)(w / 2) * (h / 2) * img; abs2 += (size_t)(w / 4) * (h / 4) * img;
    ths_smoothed += (size_t)((w / 32) * (h / 32) + 100) * img; map += (size_t)w * h * img; counts += (size_t)cstride * img;
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = gt >> 4, sub = gt & 15, lane = threadIdx.x & 63;
    const int b3 = sub >> 2, c2 = sub & 3;                            // 2pot block inside the 4pot block, cell inside the 2pot block
    int n2 = 0, n3 = 0, n4 = 0;
    bool q0 = false, q1 = false, q2 = false;
    int best0 = -1, best1 = -1, best2 = -1; float val0 = 0.f, val1 = 0.f, val2 = 0.f;
    if (b < nbx * nby) {
        const int x4 = (b % nbx) * 4 * pot, y4 = (b / nbx) * 4 * pot;
        const int x0 = x4 + (b3 & 1) * 2 * pot + (c2 & 1) * pot, y0 = y4 + (b3 >> 1) * 2 * pot + (c2 >> 1) * pot;
        const int w1 = w / 2, w2 = w / 4, w32 = w / 32;
        const float dw1 = 0.75f, dw2 = dw1 * dw1;                     // setting_gradDownweightPerLevel
        const int my1 = min(pot, h - y0), mx1 = min(pot, w - x0);
        for (int y1 = 0; y1 < my1; ++y1) for (int x1 = 0; x1 < mx1; ++x1) {
            const int xf = x1 + x0, yf = y1 + y0, idx = xf + w * yf;
            if (xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4) continue;
            const float th0 = ths_smoothed[(xf >> 5) + (yf >> 5) * w32];   // rows past h/32 read the zeroed slack, like the reference
            const float th1 = th0 * dw1, th2 = th1 * dw2;
            const float ag0 = abs0[idx];
            const float ag1 = abs1[(int)(xf * 0.5f + 0.25f) + (int)(yf * 0.5f + 0.25f) * w1];
            const float ag2 = abs2[(int)(xf * 0.25f + 0.125f) + (int)(yf * 0.25f + 0.125f) * w2];
            if (ag0 > th0) { q0 = true; if (ag0 > val0) { val0 = ag0; best0 = idx; } }
            if (ag1 > th1) { q1 = true; if (ag1 > val1) { val1 = ag1; best1 = idx; } }
            if (ag2 > th2) { q2 = true; if (ag2 > val2) { val2 = ag2; best2 = idx; } }
        }
        if (best0 > 0) { map[best0] = 1; ++n2; }
    }
    // level 1: the first lane of every group of 4 walks its group's cells in order
    const int g4 = lane & ~3, g16 = lane & ~15;
    bool any0_4 = false; int pick1 = -1; float pv1 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool k0 = __shfl((int)q0, g4 + k, 64) != 0, k1 = __shfl((int)q1, g4 + k, 64) != 0;
        const float v = __shfl(val1, g4 + k, 64); const int ix = __shfl(best1, g4 + k, 64);
        any0_4 |= k0;
        if (k1 && v > pv1) { pv1 = v; pick1 = ix; }
    }
    if (c2 == 0 && !any0_4 && pick1 > 0) { map[pick1] = 2; ++n3; }
    // level 2: the first lane of every group of 16
    bool any01_16 = false; int pick2 = -1; float pv2 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool k01 = (__shfl((int)q0, g16 + k, 64) | __shfl((int)q1, g16 + k, 64)) != 0, k2 = __shfl((int)q2, g16 + k, 64) != 0;
        const float v = __shfl(val2, g16 + k, 64); const int ix = __shfl(best2, g16 + k, 64);
        any01_16 |= k01;
        if (k2 && v > pv2) { pv2 = v; pick2 = ix; }
    }
    if (sub == 0 && !any01_16 && pick2 > 0) { map[pick2] = 4; ++n4; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { n2 += __shfl_xor(n2, off, 64); n3 += __shfl_xor(n3, off, 64); n4 += __shfl_xor(n4, off, 64); }
    if (lane == 0) { atomicAdd(&counts[0], n2); atomicAdd(&counts[1], n3); atomicAdd(&counts[2], n4); }
}

// ---- makeMaps' potential / re-selection state machine (PixelSelector2.cpp:186-229), a fresh selector per frame as in Engine::generate_pcd:
// the first pass ran at potential 3 with one re-selection allowed.  One thread per image; f32 arithmetic exactly as the host writes it
// (-ffp-contract=off, IEEE division and square root: num_have == 0 gives quotia = inf and a re-selection at potential 1).
__global__ void pcd_decide_kernel(PcdImgRec* __restrict__ rec, int n_img, int num_want) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const int pot = 3;
    const float num_want_f = (float)num_want;
    const float num_have = (float)(rec[i].sel1[0] + rec[i].sel1[1] + rec[i].sel1[2]);   // :191
    const float quotia = num_want_f / num_have;                     // :192
    const float K = num_have * (pot + 1) * (pot + 1);               // :195
    int ideal = (int)(sqrtf(K / num_want_f) - 1);                   // :196
    if (ideal < 1) ideal = 1;
    int pot2 = 0;
    if (quotia > 1.25 && pot > 1) {                                 // :199-213
        if (ideal >= pot) ideal = pot - 1;
        pot2 = ideal;
    } else if (quotia < 0.25) {                                     // :214-229
        if (ideal <= pot) ideal = pot + 1;
        pot2 = ideal;
    }
    rec[i].pot2 = pot2;
}
// an image that re-selects starts from an empty map again
__global__ void pcd_reclear_kernel(uint8_t* __restrict__ map, int n, const PcdImgRec* __restrict__ rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || rec[blockIdx.y].pot2 == 0) return;
    map[(size_t)n * blockIdx.y + i] = 0;
}
// the sub-sampling of the last selection (:252-268), from its counts
__device__ __forceinline__ void pcd_subsample_rule(const PcdImgRec& r, int num_want, int& subsample, int& char_th) {
    const int* c = r.pot2 ? r.sel2 : r.sel1;
    const float num_have = (float)(c[0] + c[1] + c[2]);
    const float quotia = (float)num_want / num_have;
    subsample = (quotia < 0.95) ? 1 : 0;
    char_th = subsample ? (int)(unsigned char)(255 * quotia) : 255;
}

// ---- makeMaps sub-sampling (PixelSelector2.cpp:252-268) + get_points_from_pixels' filter (pcd_generator.cpp:471), order
// preserving and coalesced: a workgroup owns a tile of PCD_TILE consecutive pixels, its waves take 64 consecutive pixels at a
// time (ballot + popcount give every marked pixel its rank), tiles are chained by per-tile counts (a tile adds up the counts
// of the tiles before it: there are only w*h/4096 of them).
//   pass 1  marked pixels per tile
//   pass 2  rank among ALL marked pixels -> position in the random byte pattern -> dropped pixels leave the map;
//           per tile: pixels kept, and kept with a valid depth
//   pass 3  (the cloud is allocated by then) rank among the kept, valid pixels = index of the point: planes + pixel list
constexpr int PCD_TILE = 4096;
constexpr int PCD_TILE_THREADS = 256;

struct PcdCam { float scaling_factor, fx, fy, cx, cy; };


// exclusive prefix of `flag` over the workgroup's current 256 pixels, in pixel order; `run` carries on across chunks
__device__ __forceinline__ int chunk_rank(bool flag, int* wsum, int& run) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = run, all = 0;
#pragma unroll
    for (int k = 0; k < PCD_TILE_THREADS / 64; ++k) { const int c = wsum[k]; if (k < wave) before += c; all += c; }
    __syncthreads();
    run += all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ int tiles_before(const int* counts, int tile, int* lds) {
    int v = 0;
    for (int k = threadIdx.x; k < tile; k += PCD_TILE_THREADS) v += counts[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < PCD_TILE_THREADS / 64; ++k) s += lds[k];
    __syncthreads();
    return s;
}

// (batches: image blockIdx.y's tile counts at 3 * tiles * image, its map and depth image at w * h * image)
__global__ __launch_bounds__(PCD_TILE_THREADS) void pcd_count_marked_kernel(const uint8_t* __restrict__ map, int n, int* __restrict__ tile_marked) {
    __shared__ int wsum[PCD_TILE_THREADS / 64];
    const int base = blockIdx.x * PCD_TILE, nt = (n + PCD_TILE - 1) / PCD_TILE;
    map += (size_t)n * blockIdx.y; tile_marked += (size_t)3 * nt * blockIdx.y;
    int cnt = 0;
    for (int k = threadIdx.x; k < PCD_TILE; k += PCD_TILE_THREADS) { const int i = base + k; cnt += (i < n && map[i] != 0) ? 1 : 0; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < PCD_TILE_THREADS / 64; ++k) s += wsum[k]; tile_marked[blockIdx.x] = s; }
}

// rec (not null, batches): each image's subsample / char_th follow from its own counts, and the arguments are ignored
__global__ __launch_bounds__(PCD_TILE_THREADS) void pcd_subsample_kernel(uint8_t* __restrict__ map, const uint8_t* __restrict__ pattern, int subsample, int char_th,
                                                                         const PcdImgRec* __restrict__ rec, int num_want,
                                                                         const uint16_t* __restrict__ depth, int n, const int* __restrict__ tile_marked,
                                                                         int* __restrict__ tile_valid, int* __restrict__ tile_kept) {
    __shared__ int wsum[PCD_TILE_THREADS / 64];
    const int base = blockIdx.x * PCD_TILE, nt = (n + PCD_TILE - 1) / PCD_TILE, img = blockIdx.y;
    if (rec) pcd_subsample_rule(rec[img], num_want, subsample, char_th);
    const size_t to = (size_t)3 * nt * img;
    map += (size_t)n * img; depth += (size_t)n * img; tile_marked += to; tile_valid += to; tile_kept += to;
    int run = tiles_before(tile_marked, blockIdx.x, wsum);            // marked pixels in front of this tile = index into the byte pattern
    int valid = 0, kept = 0;
    for (int k0 = 0; k0 < PCD_TILE; k0 += PCD_TILE_THREADS) {
        const int i = base + k0 + threadIdx.x;
        const bool marked = i < n && map[i] != 0;
        const int rn = chunk_rank(marked, wsum, run);
        if (marked) {
            const bool keep = !(subsample && pattern[rn] > char_th);  // PixelSelector2.cpp:261-265
            if (!keep) map[i] = 0;
            else { ++kept; valid += depth[i] != 0; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { valid += __shfl_xor(valid, off, 64); kept += __shfl_xor(kept, off, 64); }
    __shared__ int red[2][PCD_TILE_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = valid; red[1][threadIdx.x >> 6] = kept; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int k = 0; k < PCD_TILE_THREADS / 64; ++k) { a += red[0][k]; b += red[1][k]; }
        tile_valid[blockIdx.x] = a; tile_kept[blockIdx.x] = b;
    }
}

// rec (not null, batches): the point count comes from the image's tile counts (and goes to rec), the cloud to the image's slot of `cap`
// points (a count above cap writes nothing: the host refuses the call), and the points sampled for Cloud::cost_hint add up in rec.
// cams (not null, batches of several cameras: cvo_batch_advance_images): image blockIdx.y is back-projected with cams[blockIdx.y], else with cam0
__global__ __launch_bounds__(PCD_TILE_THREADS) void pcd_cloud_kernel(const uint8_t* __restrict__ map, const uint16_t* __restrict__ depth, const uint8_t* __restrict__ bgr,
                                                                     const float* __restrict__ dx0, const float* __restrict__ dy0, int w, int n, PcdCam cam0,
                                                                     const PcdCam* __restrict__ cams,
                                                                     const int* __restrict__ tile_valid, int n_points, float* __restrict__ cloud,
                                                                     uint16_t* __restrict__ px, PcdImgRec* __restrict__ rec, int cap) {
    __shared__ int wsum[PCD_TILE_THREADS / 64];
    const int base = blockIdx.x * PCD_TILE, nt = (n + PCD_TILE - 1) / PCD_TILE, img = blockIdx.y;
    const PcdCam cam = cams ? cams[img] : cam0;
    map += (size_t)n * img; depth += (size_t)n * img; bgr += (size_t)3 * n * img; dx0 += (size_t)n * img; dy0 += (size_t)n * img;
    tile_valid += (size_t)3 * nt * img;
    if (rec) {
        n_points = tiles_before(tile_valid, nt, wsum);
        if (blockIdx.x == 0 && threadIdx.x == 0) rec[img].npts = n_points;
        if (n_points > cap) return;                                   // (uniform)
        cloud += (size_t)cap * REC * img; px += (size_t)cap * 2 * img;
    }
    double cost = 0.0; int cost_n = 0;
    int run = tiles_before(tile_valid, blockIdx.x, wsum);
    for (int k0 = 0; k0 < PCD_TILE; k0 += PCD_TILE_THREADS) {
        const int i = base + k0 + threadIdx.x;
        const int dep = i < n ? (int)depth[i] : 0;
        const bool ok = i < n && map[i] != 0 && dep != 0;             // pcd_generator.cpp:471
        const int at = chunk_rank(ok, wsum, run);
        if (ok && at < n_points) {
            const int x = i % w, y = i / w;
            const float p2 = (float)dep / cam.scaling_factor;         // pcd_generator.cpp:473-476
            const float p0 = ((float)x - cam.cx) * p2 / cam.fx;
            const float p1 = ((float)y - cam.cy) * p2 / cam.fy;
            float* lo = cloud + lo_off(at); float* hi = cloud + hi_off(n_points, at);
            lo[0] = p0; lo[1] = p1; lo[2] = p2; lo[3] = (float)bgr[3 * (size_t)i];               // B  (:601)
            hi[0] = (float)bgr[3 * (size_t)i + 1]; hi[1] = (float)bgr[3 * (size_t)i + 2];        // G, R
            hi[2] = dx0[i]; hi[3] = dy0[i];                                                      // :608-609
            px[2 * at] = (uint16_t)x; px[2 * at + 1] = (uint16_t)y;
            if (rec && (at & 15) == 0 && p2 > 1e-3f) { cost += 1.0 / ((double)p2 * p2); ++cost_n; }   // Engine::upload_many's sample
        }
    }
    if (rec) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { cost += __shfl_xor(cost, off, 64); cost_n += __shfl_xor(cost_n, off, 64); }
        if ((threadIdx.x & 63) == 0 && cost_n > 0) { atomicAdd(&rec[img].cost, cost); atomicAdd(&rec[img].cost_n, cost_n); }
    }
}

// each pair's cloud of a batch from its image's slot: two planes of n float4 and n pixel pairs, one workgroup row (grid.y) per cloud
__global__ __launch_bounds__(256) void pcd_scatter_kernel(PcdScatter S) {
    const int k = blockIdx.y, im = S.img[k], np = S.rec[im].npts;
    if (np > S.cap) return;
    const float4* src = reinterpret_cast<const float4*>(S.src + (size_t)S.cap * REC * im);
    const unsigned* spx = reinterpret_cast<const unsigned*>(S.src_px + (size_t)S.cap * 2 * im);
    float4* dst = reinterpret_cast<float4*>(S.dst[k]); unsigned* dpx = reinterpret_cast<unsigned*>(S.dst_px[k]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * np; i += gridDim.x * 256) dst[i] = src[i];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < np; i += gridDim.x * 256) dpx[i] = spx[i];
}

// ---- caller-owned device images into the generator's packed stacks (cvo_*_device_images, cvo_tracks_*_device_async): image k's colour plane
// to bgr_stack + 3 n k (B, G, R per pixel), its depth plane to depth_stack + 2 n k bytes, n = w * h.  Both planes are one gather of bytes:
// output byte j of a plane with `ob` output bytes per pixel (3 / 2) comes from pixel p = j / ob, (x, y) = (p % w, p / w), source byte
// y * pitch + x * pb + c (pb source bytes per pixel, c = j % ob, mirrored for swap_rb).  A lane owns one 16-byte-aligned piece of the output,
// consecutive lanes consecutive pieces: a piece that lies wholly inside the image's plane is one 16-byte store, the plane's head and tail
// pieces (3 n k is a multiple of 16 for few k) are stored byte by byte.  A source whose base and pitch are multiples of 4 is read as whole
// dwords, each fetched once per lane; the last dword of a row, when the row's bytes end inside it, and every other source is read as bytes:
// nothing outside [row start, row start + w * pb) is touched.  Which path an image takes follows from its descriptor alone (wave-uniform).
__device__ __forceinline__ unsigned ingest_byte(const uint8_t* row, unsigned off, unsigned row_bytes, bool dwords, unsigned& at, unsigned& v) {
    if (!dwords) return row[off];
    const unsigned o4 = off & ~3u;
    if (o4 != at) {
        at = o4;
        if (o4 + 4 <= row_bytes) v = *reinterpret_cast<const unsigned*>(row + o4);
        else { v = 0; for (unsigned q = 0; o4 + q < row_bytes; ++q) v |= (unsigned)row[o4 + q] << (8 * q); }
    }
    return (v >> (8 * (off & 3u))) & 0xffu;
}
// grid: (pieces of the colour plane + pieces of the depth plane, images); pieces_* = the plane's bytes / 16 rounded up, + 1 for a plane that
// starts inside a piece
__global__ __launch_bounds__(256) void pcd_ingest_images_kernel(const PcdIngestDesc* __restrict__ descs, uint8_t* __restrict__ bgr_stack,
                                                                uint8_t* __restrict__ depth_stack, int w, unsigned n, unsigned pieces_bgr, unsigned pieces_depth) {
    const unsigned k = blockIdx.y;
    unsigned t = blockIdx.x * 256u + threadIdx.x;
    const bool is_depth = t >= pieces_bgr;
    if (is_depth) { t -= pieces_bgr; if (t >= pieces_depth) return; }
    const PcdIngestDesc D = descs[k];
    const unsigned ob = is_depth ? 2u : 3u, pb = is_depth ? 2u : (unsigned)D.pixel_bytes;
    const bool swap = !is_depth && D.swap_rb != 0, dwords = (is_depth ? D.depth_dwords : D.bgr_dwords) != 0;
    const long long pitch = is_depth ? D.depth_pitch : D.bgr_pitch;
    const uint8_t* src = is_depth ? D.depth : D.bgr;
    uint8_t* out = (is_depth ? depth_stack : bgr_stack) + (size_t)ob * n * k;
    const unsigned len = ob * n, row_bytes = pb * (unsigned)w;
    // the piece: 16 bytes at a 16-byte-aligned address, [lo, hi) of it inside the plane (byte offsets from the plane's start; lo0 may lie before it)
    const long long lo0 = 16ll * t - (long long)(reinterpret_cast<uintptr_t>(out) & 15u);
    if (lo0 >= (long long)len) return;
    const unsigned lo = lo0 < 0 ? 0u : (unsigned)lo0, hi = lo0 + 16 > (long long)len ? len : (unsigned)(lo0 + 16);
    const unsigned p = lo / ob;
    unsigned c = lo - p * ob, y = p / (unsigned)w, x = p - y * (unsigned)w;
    const uint8_t* row = src + (long long)y * pitch;
    unsigned at = 0xffffffffu, v = 0, word[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const long long j = lo0 + q;
        if (j >= (long long)lo && j < (long long)hi) {
            const unsigned byte = ingest_byte(row, x * pb + (swap ? 2u - c : c), row_bytes, dwords, at, v);
            word[q >> 2] |= byte << (8 * (q & 3));
            if (++c == ob) { c = 0; if (++x == (unsigned)w) { x = 0; row += pitch; at = 0xffffffffu; } }
        }
    }
    if (hi - lo == 16u) {
        *reinterpret_cast<uint4*>(out + lo) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long j = lo0 + q;
            if (j >= (long long)lo && j < (long long)hi) out[j] = (uint8_t)(word[q >> 2] >> (8 * (q & 3)));
        }
    }
}
hipError_t pcd_launch_ingest(const PcdIngestDesc* descs, uint8_t* bgr_stack, uint8_t* depth_stack, int w, int h, int n_img, hipStream_t s) {
    const unsigned n = (unsigned)w * (unsigned)h;
    const unsigned pieces_bgr = (3u * n + 15u) / 16u + 1u, pieces_depth = (2u * n + 15u) / 16u + 1u;
    hipLaunchKernelGGL(pcd_ingest_images_kernel, dim3((pieces_bgr + pieces_depth + 255u) / 256u, n_img), dim3(256), 0, s, descs, bgr_stack, depth_stack, w, n,
                       pieces_bgr, pieces_depth);
    return hipGetLastError();
}

// cloud planes back to the reference layout (tests, get_*_selected_points callers)
__global__ void pcd_unpack_kernel(const float* __restrict__ cloud, int n, float* __restrict__ xyz, float* __restrict__ feat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* lo = cloud + lo_off(i); const float* hi = cloud + hi_off(n, i);
    xyz[3 * (size_t)i] = lo[0]; xyz[3 * (size_t)i + 1] = lo[1]; xyz[3 * (size_t)i + 2] = lo[2];
    feat[i] = lo[3]; feat[(size_t)n + i] = hi[0]; feat[2 * (size_t)n + i] = hi[1]; feat[3 * (size_t)n + i] = hi[2]; feat[4 * (size_t)n + i] = hi[3];
}

// host clouds in the reference layout (n x 3 positions AoS, data_type.h:30; 5 channel-major feature arrays of n, data_type.h:75), copied
// to the device as they are, into the cloud's two float4 planes {x, y, z, f0}, {f1..f4}: one launch for all clouds of a hand-over
// (grid.y = cloud).  The positions of 256 consecutive points are 768 consecutive floats: fetched coalesced through LDS.
__global__ __launch_bounds__(256) void cvo_pack_clouds_kernel(const float* __restrict__ raw, const PackDesc* __restrict__ descs) {
    __shared__ float pos[768];
    const PackDesc D = descs[blockIdx.y];
    const int i0 = blockIdx.x * 256, tid = threadIdx.x;
    if (i0 >= D.n) return;
    const float* xyz = raw + D.raw_off; const float* feat = D.feat_off ? raw + D.feat_off : xyz + 3 * (size_t)D.n;
    const int cnt = min(256, D.n - i0);
    for (int k = tid; k < 3 * cnt; k += 256) pos[k] = xyz[3 * (size_t)i0 + k];
    __syncthreads();
    if (tid < cnt) {
        const int i = i0 + tid;
        float4 lo, hi;
        lo.x = pos[3 * tid]; lo.y = pos[3 * tid + 1]; lo.z = pos[3 * tid + 2]; lo.w = feat[i];
        hi.x = feat[(size_t)D.n + i]; hi.y = feat[2 * (size_t)D.n + i]; hi.z = feat[3 * (size_t)D.n + i]; hi.w = feat[4 * (size_t)D.n + i];
        *reinterpret_cast<float4*>(D.dst + lo_off(i)) = lo;
        *reinterpret_cast<float4*>(D.dst + hi_off(D.n, i)) = hi;
    }
}
hipError_t launch_pack_clouds(const float* raw, const PackDesc* descs, int n_clouds, int n_max, hipStream_t s) {
    if (n_clouds > 0 && n_max > 0) hipLaunchKernelGGL(cvo_pack_clouds_kernel, dim3((n_max + 255) / 256, n_clouds), dim3(256), 0, s, raw, descs);
    return hipGetLastError();
}

// caller-owned device clouds (cvo_*_device_clouds) into the clouds' two float4 planes: one launch for all clouds of a call, grid.y = cloud,
// a block per 256 consecutive points, the descriptor table read where it lies (pinned host memory).  Each lane assembles its point's two
// float4 and writes them with two 16-byte stores.
//   positions, xyz_stride 12 (xyz_tight): the block's m = 3 * cnt floats are consecutive, src[0, m).  They are split into a head of
//     min(m, floats up to the next 16-byte boundary), a body of whole 16-byte pieces and a tail of (m - head) % 4 floats: head + body + tail
//     = m, the 16-byte loads cover src[head, head + body) only, head and tail are taken float by float.  Through LDS to the lanes.
//   positions, any other stride: lane i reads its three floats at xyz + i * xyz_stride.
//   features: feature c of point i at feat + i * point_stride + c * channel_stride, one float per lane and channel: with a point stride
//     of 4 the lanes of a wave read consecutive floats of a channel array.
// Bounds: a lane reads for a point i < n only, so the bytes read are inside [xyz, xyz + (n - 1) * xyz_stride + 12) and [feat, feat + (n - 1) *
// point_stride + 4 * channel_stride + 4) -- the extents the host has checked against the allocations -- by construction: in the tight path the
// block reads floats [3 i0, 3 i0 + 3 cnt) of the position array and 3 (i0 + cnt) <= 3 n; no load is wider than what is left of its range.
// Cost samples (Engine::upload_many's: points i % 16 == 0 with z > 1e-3f, 1.0 / ((double)z * z)): a block starts at a multiple of 256, so its
// samples are its lanes 0, 16, ..., 240; each forms its term, lane 0 adds the sixteen in lane order and writes {sum, samples} to the block's
// place in the cloud's table.  The host adds the blocks in block order: no atomics, the same bytes on every run.
__global__ __launch_bounds__(256) void cvo_ingest_clouds_kernel(const CloudIngestDesc* __restrict__ descs) {
    __shared__ __align__(16) float pos[768];
    __shared__ double term[16];
    __shared__ int sampled[16];
    const CloudIngestDesc D = descs[blockIdx.y];
    const int i0 = blockIdx.x * 256, tid = threadIdx.x;
    if (i0 >= D.n) return;                                            // (uniform over the block)
    const int cnt = min(256, D.n - i0), i = i0 + tid;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (D.xyz_tight) {
        const float* src = D.xyz + 3 * (size_t)i0;
        const int m = 3 * cnt;
        const int head = min(m, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2));
        const int body = (m - head) & ~3, tail0 = head + body;
        if (tid < head) pos[tid] = src[tid];
        if (4 * tid < body) {
            const float4 v = *reinterpret_cast<const float4*>(src + head + 4 * tid);
            float* o = pos + head + 4 * tid;
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
        if (tid < m - tail0) pos[tail0 + tid] = src[tail0 + tid];
        __syncthreads();
        if (tid < cnt) { lo.x = pos[3 * tid]; lo.y = pos[3 * tid + 1]; lo.z = pos[3 * tid + 2]; }
    } else if (tid < cnt) {
        const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(D.xyz) + (long long)i * D.xyz_stride);
        lo.x = p[0]; lo.y = p[1]; lo.z = p[2];
    }
    if (tid < cnt) {
        const char* f = reinterpret_cast<const char*>(D.feat) + (long long)i * D.feat_point_stride;
        const long long cs = D.feat_channel_stride;
        lo.w = *reinterpret_cast<const float*>(f);
        hi.x = *reinterpret_cast<const float*>(f + cs); hi.y = *reinterpret_cast<const float*>(f + 2 * cs);
        hi.z = *reinterpret_cast<const float*>(f + 3 * cs); hi.w = *reinterpret_cast<const float*>(f + 4 * cs);
        *reinterpret_cast<float4*>(D.dst + lo_off(i)) = lo;
        *reinterpret_cast<float4*>(D.dst + hi_off(D.n, i)) = hi;
    }
    if ((tid & 15) == 0) {
        const bool ok = tid < cnt && lo.z > 1e-3f;
        term[tid >> 4] = ok ? 1.0 / ((double)lo.z * (double)lo.z) : 0.0;
        sampled[tid >> 4] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0; int k = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) { if (sampled[q]) s += term[q]; k += sampled[q]; }
        D.cost[2 * blockIdx.x] = s; D.cost[2 * blockIdx.x + 1] = (double)k;
    }
}
// descs: n_clouds descriptors the device can read (pinned host memory), every cloud with n > 0; n_max: the largest n among them
hipError_t launch_ingest_clouds(const CloudIngestDesc* descs, int n_clouds, int n_max, hipStream_t s) {
    if (n_clouds > 0 && n_max > 0) hipLaunchKernelGGL(cvo_ingest_clouds_kernel, dim3((n_max + 255) / 256, n_clouds), dim3(256), 0, s, descs);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host-side launchers
#define PCD_LAUNCH_1D(kernel, n, stream, ...) hipLaunchKernelGGL(kernel, dim3(((n) + 255) / 256), dim3(256), 0, stream, __VA_ARGS__)

// n_img images one behind the other in every buffer (the strides of the kernels above); the single-frame path passes 1
#define PCD_LAUNCH_2D(kernel, n, n_img, stream, ...) hipLaunchKernelGGL(kernel, dim3(((n) + 255) / 256, (n_img)), dim3(256), 0, stream, __VA_ARGS__)

hipError_t pcd_launch_pyramid(const uint8_t* bgr, int w, int h, float* I0, float* I1, float* I2, float* dx0, float* dy0, float* abs0, float* abs1, float* abs2,
                              int n_img, hipStream_t s) {
    const int w1 = w / 2, h1 = h / 2, w2 = w1 / 2, h2 = h1 / 2;
    PCD_LAUNCH_2D(pcd_gray_kernel, w * h, n_img, s, bgr, I0, w * h);
    PCD_LAUNCH_2D(pcd_grad_kernel, w * h, n_img, s, I0, w, h, dx0, dy0, abs0);
    PCD_LAUNCH_2D(pcd_down_kernel, w1 * h1, n_img, s, I0, w * h, I1, w1, h1);
    PCD_LAUNCH_2D(pcd_grad_kernel, w1 * h1, n_img, s, I1, w1, h1, (float*)nullptr, (float*)nullptr, abs1);
    PCD_LAUNCH_2D(pcd_down_kernel, w2 * h2, n_img, s, I1, w1 * h1, I2, w2, h2);
    PCD_LAUNCH_2D(pcd_grad_kernel, w2 * h2, n_img, s, I2, w2, h2, (float*)nullptr, (float*)nullptr, abs2);
    return hipGetLastError();
}
// ths / ths_smoothed: w/32 * h/32 + 100 floats per image, the slack zeroed
hipError_t pcd_launch_thresholds(const float* abs0, int w, int h, float* ths, float* ths_smoothed, int n_img, hipStream_t s) {
    const int w32 = w / 32, h32 = h / 32;
    if (w32 * h32 > 0) {
        hipLaunchKernelGGL(pcd_hist_kernel, dim3(w32 * h32, n_img), dim3(256), 0, s, abs0, w, h, w32, ths);
        PCD_LAUNCH_2D(pcd_smooth_kernel, w32 * h32, n_img, s, ths, w32, h32, ths_smoothed);
    }
    return hipGetLastError();
}
hipError_t pcd_launch_select(const float* abs0, const float* abs1, const float* abs2, const float* ths_smoothed, int w, int h, int pot, uint8_t* map, int* counts,
                             hipStream_t s) {
    const int nb = ((w + 4 * pot - 1) / (4 * pot)) * ((h + 4 * pot - 1) / (4 * pot));
    hipLaunchKernelGGL(pcd_select_kernel, dim3((nb * 16 + 255) / 256), dim3(256), 0, s, abs0, abs1, abs2, ths_smoothed, w, h, pot, (const int*)nullptr, map, counts, 0);
    return hipGetLastError();
}
// makeMaps for n_img images on the device (rec zeroed, map zeroed): the pass at potential 3, each image's decision, the re-selection of the
// images that ask for one -- its grid sized for potential 1, the smallest a re-selection can take
hipError_t pcd_launch_select_batch(const float* abs0, const float* abs1, const float* abs2, const float* ths_smoothed, int w, int h, uint8_t* map, PcdImgRec* rec,
                                   int n_img, int num_want, hipStream_t s) {
    constexpr int RS = (int)(sizeof(PcdImgRec) / sizeof(int));
    int* r = reinterpret_cast<int*>(rec);
    const int nb3 = ((w + 11) / 12) * ((h + 11) / 12), nb1 = ((w + 3) / 4) * ((h + 3) / 4);
    hipLaunchKernelGGL(pcd_select_kernel, dim3((nb3 * 16 + 255) / 256, n_img), dim3(256), 0, s, abs0, abs1, abs2, ths_smoothed, w, h, 3, (const int*)nullptr, map,
                       r + offsetof(PcdImgRec, sel1) / sizeof(int), RS);
    PCD_LAUNCH_1D(pcd_decide_kernel, n_img, s, rec, n_img, num_want);
    PCD_LAUNCH_2D(pcd_reclear_kernel, w * h, n_img, s, map, w * h, (const PcdImgRec*)rec);
    hipLaunchKernelGGL(pcd_select_kernel, dim3((nb1 * 16 + 255) / 256, n_img), dim3(256), 0, s, abs0, abs1, abs2, ths_smoothed, w, h, 0,
                       (const int*)(r + offsetof(PcdImgRec, pot2) / sizeof(int)), map, r + offsetof(PcdImgRec, sel2) / sizeof(int), RS);
    return hipGetLastError();
}
int pcd_tiles(int w, int h) { return (w * h + PCD_TILE - 1) / PCD_TILE; }
// tile_counts: 3 arrays of pcd_tiles() ints {marked, valid, kept}
hipError_t pcd_launch_subsample(uint8_t* map, const uint8_t* pattern, int subsample, int char_th, const uint16_t* depth, int w, int h, int* tile_counts, hipStream_t s) {
    const int nt = pcd_tiles(w, h);
    hipLaunchKernelGGL(pcd_count_marked_kernel, dim3(nt), dim3(PCD_TILE_THREADS), 0, s, map, w * h, tile_counts);
    hipLaunchKernelGGL(pcd_subsample_kernel, dim3(nt), dim3(PCD_TILE_THREADS), 0, s, map, pattern, subsample, char_th, (const PcdImgRec*)nullptr, 0, depth, w * h,
                       tile_counts, tile_counts + nt, tile_counts + 2 * nt);
    return hipGetLastError();
}
// tile_counts: 3 * pcd_tiles() ints per image; each image's sub-sampling follows from its counts in rec
hipError_t pcd_launch_subsample_batch(uint8_t* map, const uint8_t* pattern, const PcdImgRec* rec, int num_want, const uint16_t* depth, int w, int h, int* tile_counts,
                                      int n_img, hipStream_t s) {
    const int nt = pcd_tiles(w, h);
    hipLaunchKernelGGL(pcd_count_marked_kernel, dim3(nt, n_img), dim3(PCD_TILE_THREADS), 0, s, map, w * h, tile_counts);
    hipLaunchKernelGGL(pcd_subsample_kernel, dim3(nt, n_img), dim3(PCD_TILE_THREADS), 0, s, map, pattern, 0, 255, rec, num_want, depth, w * h,
                       tile_counts, tile_counts + nt, tile_counts + 2 * nt);
    return hipGetLastError();
}
hipError_t pcd_launch_cloud(const uint8_t* map, const uint16_t* depth, const uint8_t* bgr, const float* dx0, const float* dy0, int w, int h, const float cam[5],
                            const int* tile_counts, int n_points, float* cloud, uint16_t* px, hipStream_t s) {
    const int nt = pcd_tiles(w, h);
    PcdCam c{cam[0], cam[1], cam[2], cam[3], cam[4]};
    hipLaunchKernelGGL(pcd_cloud_kernel, dim3(nt), dim3(PCD_TILE_THREADS), 0, s, map, depth, bgr, dx0, dy0, w, w * h, c, (const PcdCam*)nullptr, tile_counts + nt, n_points,
                       cloud, px, (PcdImgRec*)nullptr, 0);
    return hipGetLastError();
}
// every image's cloud into its slot of `cap` points (cap * REC floats, cap * 2 pixel coordinates); counts and cost samples into rec.
// cam_table (device, n_img x 5 floats, may be null): a camera per image instead of `cam` for all
hipError_t pcd_launch_cloud_batch(const uint8_t* map, const uint16_t* depth, const uint8_t* bgr, const float* dx0, const float* dy0, int w, int h, const float cam[5],
                                  const float* cam_table, const int* tile_counts, PcdImgRec* rec, int cap, float* cloud, uint16_t* px, int n_img, hipStream_t s) {
    static_assert(sizeof(PcdCam) == 5 * sizeof(float), "camera table layout");
    const int nt = pcd_tiles(w, h);
    PcdCam c{cam[0], cam[1], cam[2], cam[3], cam[4]};
    hipLaunchKernelGGL(pcd_cloud_kernel, dim3(nt, n_img), dim3(PCD_TILE_THREADS), 0, s, map, depth, bgr, dx0, dy0, w, w * h, c, reinterpret_cast<const PcdCam*>(cam_table),
                       tile_counts + nt, 0, cloud, px, rec, cap);
    return hipGetLastError();
}
hipError_t pcd_launch_scatter(const PcdScatter& S, int n_max, hipStream_t s) {
    if (S.n > 0 && n_max > 0) hipLaunchKernelGGL(pcd_scatter_kernel, dim3(min(64, (2 * n_max + 255) / 256), S.n), dim3(256), 0, s, S);
    return hipGetLastError();
}
hipError_t pcd_launch_unpack(const float* cloud, int n, float* xyz, float* feat, hipStream_t s) {
    if (n > 0) PCD_LAUNCH_1D(pcd_unpack_kernel, n, s, cloud, n, xyz, feat);
    return hipGetLastError();
}

}  // namespace cvohip
