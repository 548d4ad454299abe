// cvo_match_kernels.hip -- point matches (NOT in the reference): what a point was matched to.  The per-point support (cvo_support_kernels.hip)
// visits every inside pair (i, j) of a request -- both gates, a_ij = ck * k (cvo.cpp:423, 428-431), no a > sp_thres test -- and keeps a sum and a
// count per row; here the partner is kept too: per row the column of the largest a_ij (lowest j on a tie: an ascending sweep and a strict >),
// that value, and the a-weighted mean of the partners' points, beside the same sum and count.
//
// cvo_match_kernel has cvo_support_kernel's shape: workgroup = one wave = 64 rows, lane = row, box_sweep over ALL column groups in ascending
// order, pair arithmetic from cvo_sweep.hpp.  A lane owns its row's five f64 accumulators and its running best and stores them itself: no
// reduction, no atomics, a row's bits depend on the two clouds, the transform, ell and the parameters alone.  sum and count are the support
// kernel's own statements, so they carry its bits.  The moved plane and its boxes come from the support's pre-pass (launch_support_prepass).
//
// cvo_match_fit_kernel: one wave per request reads what the sweep wrote and the rows' own points and makes the request's fit record --
// rows, matched rows, sum of the weights and of weight x squared residual (mean - point, in float).  Lane L adds rows L, L + 64, ... in
// ascending order, then the 64 lanes are added with the xor-butterfly the other reduce kernels use.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_sweep.hpp"

namespace cvohip {

hipError_t launch_support_prepass(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, hipStream_t stream);   // cvo_support_kernels.hip

constexpr int MATCH_BLOCK = 64;

__global__ __launch_bounds__(MATCH_BLOCK) void cvo_match_kernel(const MatchDesc* __restrict__ descs, DevParams P, unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const MatchDesc& D = descs[blockIdx.z];
    if ((int)blockIdx.x * MATCH_BLOCK >= D.na) return;               // (uniform: the grid is sized for the launch's largest request)
    __shared__ __attribute__((aligned(16))) float lx[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SWEEP_STAGE];

    const int tid = threadIdx.x, i = blockIdx.x * MATCH_BLOCK + tid;
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

    double sumA = 0, m0 = 0, m1 = 0, m2 = 0; int count = 0;
    int best = -1; float best_a = -1.0f;                             // a_ij >= 0: the first inside column is taken
    box_sweep(pa, valid, D.bbox, D.nbox, 0, D.nbox, D.b_lo, D.nb, d2_thres, lx, ly, lz, [&](int j, const float (&pb)[3], float d2) {
        const float4 blo4 = ld4s(D.b_lo + lo_off(j)), bhi4 = ld4s(D.b_hi + lo_off(j));
        const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
        const float d2c = pair_d2c(fa, fb);
        if (!(d2c < d2c_thres)) return;                                      // cvo.cpp:428
        const float a = pair_ck(d2c, csig2, den_c) * pair_k(d2, sig2, den_l);    // cvo.cpp:429-431
        sumA += a; count += 1;                                               // this row's terms, ascending columns (cvo_support_kernel's)
        const double ad = (double)a;
        m0 += ad * (double)pb[0]; m1 += ad * (double)pb[1]; m2 += ad * (double)pb[2];
        if (a > best_a) { best_a = a; best = j; }                            // strict: the lowest column of a tie stays
    });
    if (valid) {
        const bool any = count > 0;                                  // a row without an inside column: -1 and zeros
        D.sum[i] = (float)sumA; D.count[i] = count;
        D.best[i] = best; D.best_value[i] = any ? best_a : 0.0f;
        D.mean[3 * (size_t)i + 0] = any ? (float)(m0 / sumA) : 0.0f;         // the quotient in double, one rounding
        D.mean[3 * (size_t)i + 1] = any ? (float)(m1 / sumA) : 0.0f;
        D.mean[3 * (size_t)i + 2] = any ? (float)(m2 / sumA) : 0.0f;
    }
}

// grid.x = request; a request without a fit record has nothing to do here
__global__ __launch_bounds__(MATCH_BLOCK) void cvo_match_fit_kernel(const MatchDesc* __restrict__ descs) {
    const MatchDesc& D = descs[blockIdx.x];
    if (!D.fit) return;
    const int lane = threadIdx.x;
    int matched = 0; double sum_w = 0, sum_w_res2 = 0;
    for (int i = lane; i < D.na; i += MATCH_BLOCK) {
        const float4 lo = ld4s(D.a_lo + lo_off(i));                  // the row's point in the fixed frame
        const float s = D.sum[i];
        const float r0 = D.mean[3 * (size_t)i + 0] - lo.x, r1 = D.mean[3 * (size_t)i + 1] - lo.y, r2 = D.mean[3 * (size_t)i + 2] - lo.z;
        const float res2 = (r0 * r0 + r1 * r1) + r2 * r2;
        matched += D.count[i] > 0 ? 1 : 0;
        sum_w += (double)s;
        sum_w_res2 += (double)s * (double)res2;                      // (an unmatched row: 0 times a finite number)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) matched += __shfl_xor(matched, off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum_w += __shfl_xor(sum_w, off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum_w_res2 += __shfl_xor(sum_w_res2, off, 64);
    if (lane == 0) { MatchFit f; f.rows = D.na; f.matched = matched; f.sum_w = sum_w; f.sum_w_res2 = sum_w_res2; *D.fit = f; }
}

int match_row_blocks(int na) { return (na + MATCH_BLOCK - 1) / MATCH_BLOCK; }

// One call's launches on `stream`, all tables in device memory: the support's pre-pass (moved planes of n_moves clouds and their group boxes), ONE
// sweep over the n_reqs requests (grid z; row_blocks = the blocks of the request with the most rows), and with_fit: the fit records behind it.
hipError_t launch_match(const SupportMoveDesc* moves, const BoxDesc* boxes, int n_moves, int n_move_max, const MatchDesc* reqs, int n_reqs, int row_blocks,
                        bool with_fit, const DevParams& P, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    hipError_t e = launch_support_prepass(moves, boxes, n_moves, n_move_max, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cvo_match_kernel, dim3(row_blocks, 1, n_reqs), dim3(MATCH_BLOCK), 0, stream, reqs, P, wgs_started);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sweep_submitted) *sweep_submitted = true;                    // its workgroups will count themselves as started
    if (with_fit) {
        hipLaunchKernelGGL(cvo_match_fit_kernel, dim3(n_reqs), dim3(MATCH_BLOCK), 0, stream, reqs);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace cvohip
