// cvo_pose_model_kernels.hip -- pose models (NOT in the reference): value, se(3) gradient and Hessian of function_inner_product's sum (cvo.cpp:388-459)
// of a pair's moving cloud under each of K transforms against its fixed cloud, all pairs and all transforms in ONE launch (include/cvo_hip.h,
// "pose models").  The hypotheses' sweep (cvo_hypothesis_kernels.hip) with the geometry kept: per inside pair the weight w = il2 * (ck * k), the
// gradient's six terms w * (pa x pb), w * (pb - pa) and the 21 second-order terms of pair_hessian_add_weighted (cvo_sweep.hpp), every term a float.
//
// cvo_pose_model_sweep_kernel: grid = (64-row blocks of the launch's largest moving cloud, K, pairs), workgroup = one wave, lane = row.  A lane adds
// its terms to 29 f64 accumulators in ascending column order, the wave adds its lanes with the butterfly cvo_hyp_score_kernel uses and writes one
// record of 29 doubles.  cvo_pose_model_reduce_kernel: one wave per (pair, transform), lane = entry: the records in ascending block order, then the
// 6 x 6 matrix from the 21 sums and S, the 1/2 hat(grad_v) of Exp's second-order term.  No atomics on any sum: the bits of a model depend on the two
// clouds, that transform, ell and the parameters and on nothing else (a block past its pair's rows writes a zero record, and x + 0.0 == x for every
// x that occurs: a sum that is -0.0 does not occur, the accumulators start at +0.0).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_sweep.hpp"

namespace cvohip {

constexpr int PM_BLOCK = 64;
constexpr int PM_TERMS = POSE_MODEL_TERMS;   // 0 sum, 1 count, 2..7 gradient (omega, v), 8..28 the 21 second-order sums (A 6, C 9, D 6)

__global__ __launch_bounds__(PM_BLOCK) void cvo_pose_model_sweep_kernel(const PoseModelDesc* __restrict__ descs, DevParams P, double* __restrict__ partials,
                                                                        unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const PoseModelDesc& D = descs[blockIdx.z];
    const int tid = threadIdx.x, i = blockIdx.x * PM_BLOCK + tid;
    const size_t rec = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if ((int)blockIdx.x * PM_BLOCK >= D.na) {                        // (uniform: the grid is sized for the launch's largest moving cloud)
        if (tid < PM_TERMS) partials[rec * PM_TERMS + tid] = 0.0;    // the reduce step reads every record of the launch
        return;
    }
    __shared__ __attribute__((aligned(16))) float lx[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SWEEP_STAGE];

    const float ell = D.from ? D.from->ell : D.ell, sigma = P.sigma;
    const float* M = D.from ? D.from->transform : D.trans + 12 * (size_t)blockIdx.y;
    const float d2_thres = gate_d2_score(ell, P.sp_thres, sigma);                // cvo.cpp:395
    const float d2c_thres = gate_d2c(P.c_ell, P.sp_thres, P.c_sigma);            // cvo.cpp:396
    const double den_l = 2.0 * ell * ell, den_c = 2.0 * P.c_ell * P.c_ell;
    const float sig2 = sigma * sigma, csig2 = P.c_sigma * P.c_sigma;
    const float il2 = 1 / (ell * ell);

    float pa[3] = {3.0e18f, 3.0e18f, 3.0e18f};
    float fa[5] = {0, 0, 0, 0, 0};
    const bool valid = i < D.na;
    if (valid) {
        const float4 lo = ld4s(D.a + lo_off(i)), hi = ld4s(D.a + hi_off(D.na, i));
        apply_transform(M, lo.x, lo.y, lo.z, pa[0], pa[1], pa[2]);   // cvo.cpp:485-487
        fa[0] = lo.w; fa[1] = hi.x; fa[2] = hi.y; fa[3] = hi.z; fa[4] = hi.w;
    }

    double sumA = 0, G[6] = {0, 0, 0, 0, 0, 0}, H[21]; int count = 0;
#pragma unroll
    for (int q = 0; q < 21; ++q) H[q] = 0;
    box_sweep(pa, valid, D.bbox, D.nbox, 0, D.nbox, D.b, D.nb, d2_thres, lx, ly, lz, [&](int j, const float (&pb)[3], float d2) {
        const float4 blo4 = ld4s(D.b + lo_off(j)), bhi4 = ld4s(D.b + hi_off(D.nb, j));
        const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
        const float d2c = pair_d2c(fa, fb);
        if (!(d2c < d2c_thres)) return;                                      // cvo.cpp:428
        const float a = pair_ck(d2c, csig2, den_c) * pair_k(d2, sig2, den_l);    // cvo.cpp:429-431
        const float w = il2 * a;                                             // the energy's own weight, where cvo.cpp:707 has il2 * cdot * k
        float cr[3], db[3];
        pair_hessian_add_weighted(pa, pb, il2, w, H, cr, db);
#pragma unroll
        for (int q = 0; q < 3; ++q) { G[q] += w * cr[q]; G[3 + q] += w * db[q]; }
        sumA += a; count += 1;                                               // this row's terms in ascending columns
    });

    double acc[PM_TERMS];
    acc[0] = sumA; acc[1] = (double)count;
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[2 + q] = G[q];
#pragma unroll
    for (int q = 0; q < 21; ++q) acc[8 + q] = H[q];
    double mine = 0;                                                 // lane q keeps entry q
#pragma unroll
    for (int q = 0; q < PM_TERMS; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        mine = (tid == q) ? v : mine;
    }
    if (tid < PM_TERMS) partials[rec * PM_TERMS + tid] = mine;
}

// One wave per (pair, transform): grid = (K, pairs).  out: pairs x K models in pinned host memory (no copy engine, as cvo_hyp_reduce_select_kernel).
__global__ __launch_bounds__(PM_BLOCK) void cvo_pose_model_reduce_kernel(const double* __restrict__ partials, int row_blocks, PoseModel* __restrict__ out) {
    __shared__ double s[PM_TERMS];
    const int e = threadIdx.x;
    const size_t m = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (e < PM_TERMS) {
        const double* r = partials + m * (size_t)row_blocks * PM_TERMS + e;
        double sum = 0;
#pragma unroll 4
        for (int blk = 0; blk < row_blocks; ++blk) sum += r[(size_t)blk * PM_TERMS];   // ascending blocks
        s[e] = sum;
    }
    __syncthreads();
    PoseModel& o = out[m];
    if (e == 0) { o.value = (float)s[0]; o.num = s[1] == 0 ? 1 : (int)s[1]; }          // cvo.cpp:455-457
    if (e < 6) o.grad[e] = s[2 + e];
    if (e < 36) {
        const int r = e / 6, c = e % 6;
        const int lo = min(r % 3, c % 3), hi = max(r % 3, c % 3);
        const int sym = lo * (5 - lo) / 2 + hi;                      // a symmetric 3 x 3 block's six sums: 00 01 02 11 12 22
        double h;
        if (r < 3 && c < 3) h = s[8 + sym];                          // A at (omega, omega)
        else if (r >= 3 && c >= 3) h = s[23 + sym];                  // D at (v, v)
        else {
            const int i = r >= 3 ? r - 3 : c - 3, j = r >= 3 ? c : r;       // C(i, j) at (v_i, omega_j), its transpose at (omega_j, v_i)
            h = s[14 + 3 * i + j];
            if (i != j) {                                            // S: 1/2 hat(grad_v)(i, j) = +-1/2 g[3 - i - j]
                const double half_g = 0.5 * s[5 + (3 - i - j)];
                h += ((j - i + 3) % 3 == 1) ? -half_g : half_g;      // hat(g) = [[0, -g2, g1], [g2, 0, -g0], [-g1, g0, 0]]
            }
        }
        o.hess[e] = h;
    }
}

int pose_model_row_blocks(int na) { return (na + PM_BLOCK - 1) / PM_BLOCK; }

// One call's two launches on `stream`: the sweep over (row_blocks, k, n_pairs) workgroups, then the reduce step.  descs: n_pairs descriptors in
// device memory; partials: n_pairs * k * row_blocks records of POSE_MODEL_TERMS doubles; out: n_pairs * k models, device-readable pinned host memory.
hipError_t launch_pose_models(const PoseModelDesc* descs, int n_pairs, int k, int row_blocks, const DevParams& P, double* partials, PoseModel* out,
                              hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    hipLaunchKernelGGL(cvo_pose_model_sweep_kernel, dim3(row_blocks, k, n_pairs), dim3(PM_BLOCK), 0, stream, descs, P, partials, wgs_started);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sweep_submitted) *sweep_submitted = true;                   // its workgroups will count themselves as started
    hipLaunchKernelGGL(cvo_pose_model_reduce_kernel, dim3(k, n_pairs), dim3(PM_BLOCK), 0, stream, partials, row_blocks, out);
    return hipGetLastError();
}

}  // namespace cvohip
