// cvo_support_kernels.hip -- per-point support (NOT in the reference): the kernel matrix that function_inner_product (cvo.cpp:388-459) sums
// into one number, kept per point.  For every row i of a request, {sum over the inside columns j of a_ij, their number}; a pair is inside
// when it passes both gates (cvo.cpp:423, 428), a_ij = ck * k (cvo.cpp:429-431), no a > sp_thres test.
//
// Sweep and pair arithmetic are cvo_sweep.hpp's (box_sweep, pair_*), as in cvo_score_kernel: workgroup = one wave = 64 rows, lane = row.
// What differs is where the terms go: a lane keeps its own f64 sum and count and stores them itself, so there is no reduction and no
// second kernel.  A wave sweeps ALL groups of the columns, in ascending order: the bits of a row depend on the two clouds, ell and the
// parameters and on nothing else -- not on the launch's shape, not on what else shares it.
//
// A request is one direction of one pair.  The other direction is the same kernel with the roles swapped, and so that a_ij is one float on
// both sides the moved rows are computed ONCE (cvo_support_move_kernel, apply_transform as the score kernel applies it) into a scratch
// {x, y, z, f0} plane both requests read: (p - q)^2 == (q - p)^2 exactly, every other operand is symmetric as written.  The scratch
// plane's group boxes are made by the clouds' own box kernel (cvo_cloud_boxes_batch_kernel): a cloud's boxes describe its unmoved points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_sweep.hpp"

namespace cvohip {

hipError_t launch_cloud_boxes_batch(const BoxDesc* descs, int n_clouds, int n_max, hipStream_t stream);   // cvo_score_kernels.hip

constexpr int SUP_BLOCK = 64;

// grid.y = cloud, grid.x = 256-point blocks of the largest one
__global__ __launch_bounds__(256) void cvo_support_move_kernel(const SupportMoveDesc* __restrict__ descs) {
    const SupportMoveDesc& D = descs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D.n) return;
    const float* M = D.from ? D.from->transform : D.tran;
    const float4 p = ld4s(D.src + lo_off(i));
    float4 y; y.w = p.w;
    apply_transform(M, p.x, p.y, p.z, y.x, y.y, y.z);               // cvo.cpp:338, 485-487
    *reinterpret_cast<float4*>(D.dst + lo_off(i)) = y;
}

__global__ __launch_bounds__(SUP_BLOCK) void cvo_support_kernel(const SupportDesc* __restrict__ descs, DevParams P, unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const SupportDesc& D = descs[blockIdx.z];
    if ((int)blockIdx.x * SUP_BLOCK >= D.na) return;                 // (uniform: the grid is sized for the launch's largest request)
    __shared__ __attribute__((aligned(16))) float lx[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SWEEP_STAGE];

    const int tid = threadIdx.x, i = blockIdx.x * SUP_BLOCK + tid;
    const float ell = D.from ? D.from->ell : D.ell, sigma = P.sigma;
    const float d2_thres = gate_d2_score(ell, P.sp_thres, sigma);                // cvo.cpp:395
    const float d2c_thres = gate_d2c(P.c_ell, P.sp_thres, P.c_sigma);            // cvo.cpp:396
    const double den_l = 2.0 * ell * ell, den_c = 2.0 * P.c_ell * P.c_ell;
    const float sig2 = sigma * sigma, csig2 = P.c_sigma * P.c_sigma;

    float pa[3] = {3.0e18f, 3.0e18f, 3.0e18f};
    float fa[5] = {0, 0, 0, 0, 0};
    const bool valid = i < D.na;
    if (valid) {
        const float4 lo = ld4s(D.a_lo + lo_off(i)), hi = ld4s(D.a_hi + lo_off(i));
        pa[0] = lo.x; pa[1] = lo.y; pa[2] = lo.z;
        fa[0] = lo.w; fa[1] = hi.x; fa[2] = hi.y; fa[3] = hi.z; fa[4] = hi.w;
    }

    double sumA = 0; int count = 0;
    box_sweep(pa, valid, D.bbox, D.nbox, 0, D.nbox, D.b_lo, D.nb, d2_thres, lx, ly, lz, [&](int j, const float (&pb)[3], float d2) {
        const float4 blo4 = ld4s(D.b_lo + lo_off(j)), bhi4 = ld4s(D.b_hi + lo_off(j));
        const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
        const float d2c = pair_d2c(fa, fb);
        if (!(d2c < d2c_thres)) return;                                      // cvo.cpp:428
        const float a = pair_ck(d2c, csig2, den_c) * pair_k(d2, sig2, den_l);    // cvo.cpp:429-431
        sumA += a; count += 1;                                               // this row's terms, ascending columns
    });
    if (valid) { D.sum[i] = (float)sumA; D.count[i] = count; }      // one rounding; a row without an inside column: 0 and 0
}

int support_row_blocks(int na) { return (na + SUP_BLOCK - 1) / SUP_BLOCK; }

// The pre-pass of a call on `stream`: the moved planes of n_moves clouds and their group boxes (none: nothing is launched).  The point matches
// (cvo_match_kernels.hip) start with the same two launches.
hipError_t launch_support_prepass(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, hipStream_t stream) {
    if (n_moves <= 0) return hipSuccess;
    hipLaunchKernelGGL(cvo_support_move_kernel, dim3((n_move_max + 255) / 256, n_moves), dim3(256), 0, stream, moves);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_cloud_boxes_batch(boxes, n_moves, n_move_max, stream);
}

// One call's launches on `stream`, all tables in device memory: the pre-pass, then ONE sweep over the n_reqs requests (grid z), row_blocks = the
// blocks of the request with the most rows.
hipError_t launch_support(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, const SupportDesc* reqs, int n_reqs, int row_blocks,
                          const DevParams& P, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    { const hipError_t e = launch_support_prepass(moves, boxes, n_moves, n_move_max, stream); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(cvo_support_kernel, dim3(row_blocks, 1, n_reqs), dim3(SUP_BLOCK), 0, stream, reqs, P, wgs_started);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && sweep_submitted) *sweep_submitted = true;   // its workgroups will count themselves as started
    return e;
}

}  // namespace cvohip
