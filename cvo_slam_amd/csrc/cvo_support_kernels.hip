// cvo_support_kernels.hip -- per-point support (NOT in the reference): the kernel matrix that function_inner_product (cvo.cpp:388-459) sums
// into one number, kept per point.  For every row i of a request, {sum over the inside columns j of a_ij, their number}; a pair is inside
// when it passes both gates (cvo.cpp:423, 428), a_ij = ck * k (cvo.cpp:429-431), no a > sp_thres test.
//
// The sweep is cvo_score_kernel's (cvo_score_kernels.hip): workgroup = one wave = 64 rows, lane = row; the rows' box against the boxes of the
// columns' 32-point groups, 64 groups per ballot; up to four near groups staged in LDS (every lane reads the same 16 bytes: a broadcast) and
// swept with the fused test; a hit re-tested with the reference's un-fused d2 (nanoflann.hpp:403-406) and its features fetched only then;
// double exp, float product.  What differs is where the terms go: a lane keeps its own f64 sum and count and stores them itself, so there
// is no reduction and no second kernel.  A wave sweeps ALL groups of the columns, in ascending order: the bits of a row depend on the two
// clouds, ell and the parameters and on nothing else -- not on the launch's shape, not on what else shares it.
//
// A request is one direction of one pair.  The other direction is the same kernel with the roles swapped, and so that a_ij is one float on
// both sides the moved rows are computed ONCE (cvo_support_move_kernel, apply_transform as the score kernel applies it) into a scratch
// {x, y, z, f0} plane both requests read: (p - q)^2 == (q - p)^2 exactly, every other operand is symmetric as written.  The scratch
// plane's group boxes are made by the clouds' own box kernel (cvo_cloud_boxes_batch_kernel): a cloud's boxes describe its unmoved points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"

namespace cvohip {

hipError_t launch_cloud_boxes_batch(const BoxDesc* descs, int n_clouds, int n_max, hipStream_t stream);   // cvo_score_kernels.hip

namespace {
constexpr int SUP_BLOCK = 64;
constexpr int SUP_STAGE = 4;       // near groups fetched per round
__device__ __forceinline__ float4 sld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float swmin(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float swmax(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
}  // namespace

// grid.y = cloud, grid.x = 256-point blocks of the largest one
__global__ __launch_bounds__(256) void cvo_support_move_kernel(const SupportMoveDesc* __restrict__ descs) {
    const SupportMoveDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D.n) return;
    const float* M = D.from ? D.from->transform : D.tran;
    const float4 p = sld4(D.src + lo_off(i));
    float4 y; y.w = p.w;
    apply_transform(M, p.x, p.y, p.z, y.x, y.y, y.z);               // cvo.cpp:338, 485-487
    *reinterpret_cast<float4*>(D.dst + lo_off(i)) = y;
}

__global__ __launch_bounds__(SUP_BLOCK) void cvo_support_kernel(const SupportDesc* __restrict__ descs, DevParams P, unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const SupportDesc& D = descs[blockIdx.z];
    if ((int)blockIdx.x * SUP_BLOCK >= D.na) return;                 // (uniform: the grid is sized for the launch's largest request)
    __shared__ __attribute__((aligned(16))) float lx[32 * SUP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SUP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SUP_STAGE];

    const int tid = threadIdx.x, i = blockIdx.x * SUP_BLOCK + tid;
    const float ell = D.from ? D.from->ell : D.ell, sigma = P.sigma;
    const float d2_thres = gate_d2_score(ell, P.sp_thres, sigma);                // cvo.cpp:395
    const float d2c_thres = gate_d2c(P.c_ell, P.sp_thres, P.c_sigma);            // cvo.cpp:396
    const float thr_cull = d2_thres * (1.0f + 1e-6f);
    const float thr_box = thr_cull * 1.001f;                                     // box gaps are compared with a margin: a skipped group holds no hit
    const float Rb = sqrtf(fmaxf(thr_cull, 0.f));
    const double den_l = 2.0 * ell * ell, den_c = 2.0 * P.c_ell * P.c_ell;
    const float sig2 = sigma * sigma, csig2 = P.c_sigma * P.c_sigma;
    const float INF = __builtin_inff();

    float pa[3] = {3.0e18f, 3.0e18f, 3.0e18f};
    float fa[5] = {0, 0, 0, 0, 0};
    float blo[4] = {INF, INF, INF, INF}, bhi[4] = {-INF, -INF, -INF, -INF};
    const bool valid = i < D.na;
    if (valid) {
        const float4 lo = sld4(D.a_lo + lo_off(i)), hi = sld4(D.a_hi + lo_off(i));
        pa[0] = lo.x; pa[1] = lo.y; pa[2] = lo.z;
        fa[0] = lo.w; fa[1] = hi.x; fa[2] = hi.y; fa[3] = hi.z; fa[4] = hi.w;
#pragma unroll
        for (int q = 0; q < 3; ++q) blo[q] = bhi[q] = pa[q];
        if (pa[2] > 1.0e-3f) { blo[3] = bhi[3] = pa[1] / pa[2]; } else { blo[3] = -INF; bhi[3] = INF; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { blo[q] = swmin(blo[q]); bhi[q] = swmax(bhi[q]); }
    // points p (a row), q (a column) within Rb of each other: |y_p/z_p - y_q/z_q| <= Rb (1 + |y_q/z_q|) / z_p
    const float slope_reach = (blo[2] > 1.0e-3f) ? Rb * 1.01f / blo[2] : INF;
    const float nthr = -thr_cull;

    double sumA = 0; int count = 0;

    const int ngroups = D.nbox;
    for (int gb = 0; gb < ngroups; gb += 64) {
        bool near = false;
        if (gb + tid < ngroups) {
            float gap2 = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float glo = D.bbox[q * ngroups + gb + tid], ghi = D.bbox[(4 + q) * ngroups + gb + tid];
                const float d = fmaxf(0.f, fmaxf(glo - bhi[q], blo[q] - ghi));
                gap2 = __builtin_fmaf(d, d, gap2);
            }
            const float tlo = D.bbox[3 * ngroups + gb + tid], thi = D.bbox[7 * ngroups + gb + tid];
            const float tgap = fmaxf(0.f, fmaxf(tlo - bhi[3], blo[3] - thi));
            const float tabs = fmaxf(fabsf(tlo), fabsf(thi));
            near = (gap2 <= thr_box) && (tgap <= slope_reach * (1.0f + tabs) + 1.0e-6f);   // false for NaN (inf - inf)
        }
        unsigned long long mask = __ballot(near);
        while (mask) {
            // up to SUP_STAGE near groups are fetched together (their loads overlap), then swept one after the other
            int gis[SUP_STAGE]; int ns = 0;
#pragma unroll
            for (int k = 0; k < SUP_STAGE; ++k) {
                gis[k] = -1;
                if (mask) { gis[k] = gb + __builtin_ctzll(mask); mask &= mask - 1ull; ns = k + 1; }
            }
            __syncthreads();                                        // the previous groups have been swept
#pragma unroll
            for (int pass = 0; pass < SUP_STAGE / 2; ++pass) {
                const int gsel = (tid >> 5) ? gis[2 * pass + 1] : gis[2 * pass];
                if (gsel >= 0) {
                    const int j = gsel * 32 + (tid & 31);
                    float b0 = -3.0e18f, b1 = -3.0e18f, b2 = -3.0e18f;
                    if (j < D.nb) { const float4 lo = sld4(D.b_lo + lo_off(j)); b0 = lo.x; b1 = lo.y; b2 = lo.z; }
                    lx[pass * 64 + tid] = b0; ly[pass * 64 + tid] = b1; lz[pass * 64 + tid] = b2;
                }
            }
            __syncthreads();
            for (int k = 0; k < ns; ++k) {
                int gi = gis[0];
#pragma unroll
                for (int k2 = 1; k2 < SUP_STAGE; ++k2) gi = (k == k2) ? gis[k2] : gi;
                uint32_t w = 0u;
                const float4* qx = reinterpret_cast<const float4*>(lx + k * 32);
                const float4* qy = reinterpret_cast<const float4*>(ly + k * 32);
                const float4* qz = reinterpret_cast<const float4*>(lz + k * 32);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float4 X = qx[q], Y = qy[q], Z = qz[q];
                    const float cx[4] = {X.x, X.y, X.z, X.w}, cy[4] = {Y.x, Y.y, Y.z, Y.w}, cz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float dx = pa[0] - cx[u], dy = pa[1] - cy[u], dz = pa[2] - cz[u];
                        const float t = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, nthr)));
                        w = __builtin_amdgcn_alignbit(w, __float_as_uint(t), 31);     // sign bit: inside the (slightly widened) radius
                    }
                }
                while (w) {                                             // bit 31 = first column of the group: ascending columns
                    const int kbit = __clz(w);
                    w &= ~(0x80000000u >> kbit);
                    const int j = gi * 32 + kbit;
                    const float pb[3] = {lx[k * 32 + kbit], ly[k * 32 + kbit], lz[k * 32 + kbit]};
                    const float e0 = pa[0] - pb[0], e1 = pa[1] - pb[1], e2 = pa[2] - pb[2];
                    float d2 = e0 * e0; d2 = d2 + e1 * e1; d2 = d2 + e2 * e2;            // nanoflann.hpp:403-406
                    if (!(d2 < d2_thres)) continue;                                      // cvo.cpp:423
                    const float4 blo4 = sld4(D.b_lo + lo_off(j)), bhi4 = sld4(D.b_hi + lo_off(j));
                    const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
                    float t[5];
#pragma unroll
                    for (int c = 0; c < 5; ++c) { const float e = fa[c] - fb[c]; t[c] = e * e; }
                    const float d2c = (t[0] + t[1]) + (t[2] + (t[3] + t[4]));
                    if (!(d2c < d2c_thres)) continue;                                    // cvo.cpp:428
                    const float kk = (float)((double)sig2 * exp((double)(-d2) / den_l)); // cvo.cpp:429
                    const float ck = (float)((double)csig2 * exp((double)(-d2c) / den_c));   // cvo.cpp:430
                    const float a = ck * kk;
                    sumA += a; count += 1;                                               // this row's terms, ascending columns
                }
            }
        }
    }
    if (valid) { D.sum[i] = (float)sumA; D.count[i] = count; }      // one rounding; a row without an inside column: 0 and 0
}

int support_row_blocks(int na) { return (na + SUP_BLOCK - 1) / SUP_BLOCK; }

// One call's launches on `stream`, all tables in device memory: the moved planes of n_moves clouds and their group boxes, then ONE sweep over
// the n_reqs requests (grid z), row_blocks = the blocks of the request with the most rows.
hipError_t launch_support(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, const SupportDesc* reqs, int n_reqs, int row_blocks,
                          const DevParams& P, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    if (n_moves > 0) {
        hipLaunchKernelGGL(cvo_support_move_kernel, dim3((n_move_max + 255) / 256, n_moves), dim3(256), 0, stream, moves);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if ((e = launch_cloud_boxes_batch(boxes, n_moves, n_move_max, stream)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cvo_support_kernel, dim3(row_blocks, 1, n_reqs), dim3(SUP_BLOCK), 0, stream, reqs, P, wgs_started);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && sweep_submitted) *sweep_submitted = true;   // its workgroups will count themselves as started
    return e;
}

}  // namespace cvohip
