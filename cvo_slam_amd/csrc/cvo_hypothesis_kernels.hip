// cvo_hypothesis_kernels.hip -- pose hypotheses (NOT in the reference): function_inner_product (cvo.cpp:388-459) of a pair's moving cloud under
// each of K candidate transforms against its fixed cloud, all pairs and all hypotheses in ONE launch, and -- for a seeding call -- the pair's best
// hypothesis written as its device-resident start state, so that an align launch queued right behind starts from it (include/cvo_hip.h,
// "pose hypotheses").
//
// cvo_hyp_score_kernel: grid = (64-row blocks of the launch's largest moving cloud, K, pairs), workgroup = one wave, lane = row.  Sweep and pair
// arithmetic are cvo_sweep.hpp's (box_sweep, pair_*), the transform is applied by apply_transform as cvo_score_kernel applies it.  A wave sweeps
// ALL column groups in ascending order (no column chunks), adds its lanes' f64 sums and counts with the butterfly cvo_score_kernel uses and
// writes one {sum, count} record.  cvo_hyp_reduce_select_kernel: one wave per pair, lane = hypothesis; a lane adds its hypothesis' records in
// ascending block order and rounds once, then the wave picks the lowest index among the largest values.  No atomics on any sum: the bits of a
// (pair, hypothesis) depend on the two clouds, that transform, ell and the parameters and on nothing else -- not on K, the hypothesis' place,
// the other pairs of the launch or the grid (a block past its pair's rows writes a zero record, and x + 0.0 == x for every x that occurs).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_sweep.hpp"

namespace cvohip {

constexpr int HYP_BLOCK = 64;
constexpr int HYP_MAX = 64;        // hypotheses per pair: one lane each in the select step (CVO_MAX_HYPOTHESES)

__global__ __launch_bounds__(HYP_BLOCK) void cvo_hyp_score_kernel(const HypDesc* __restrict__ descs, DevParams P, double* __restrict__ partials,
                                                                   unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const HypDesc& D = descs[blockIdx.z];
    const int tid = threadIdx.x, i = blockIdx.x * HYP_BLOCK + tid;
    const size_t rec = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if ((int)blockIdx.x * HYP_BLOCK >= D.na) {                       // (uniform: the grid is sized for the launch's largest moving cloud)
        if (tid < 2) partials[rec * 2 + tid] = 0.0;                  // the reduce step reads every record of the launch
        return;
    }
    __shared__ __attribute__((aligned(16))) float lx[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SWEEP_STAGE];

    const float ell = D.ell, sigma = P.sigma;
    const float d2_thres = gate_d2_score(ell, P.sp_thres, sigma);                // cvo.cpp:395
    const float d2c_thres = gate_d2c(P.c_ell, P.sp_thres, P.c_sigma);            // cvo.cpp:396
    const double den_l = 2.0 * ell * ell, den_c = 2.0 * P.c_ell * P.c_ell;
    const float sig2 = sigma * sigma, csig2 = P.c_sigma * P.c_sigma;

    float pa[3] = {3.0e18f, 3.0e18f, 3.0e18f};
    float fa[5] = {0, 0, 0, 0, 0};
    const bool valid = i < D.na;
    if (valid) {
        const float4 lo = ld4s(D.a + lo_off(i)), hi = ld4s(D.a + hi_off(D.na, i));
        apply_transform(D.trans + 12 * (size_t)blockIdx.y, lo.x, lo.y, lo.z, pa[0], pa[1], pa[2]);   // cvo.cpp:485-487
        fa[0] = lo.w; fa[1] = hi.x; fa[2] = hi.y; fa[3] = hi.z; fa[4] = hi.w;
    }

    double sumA = 0; int count = 0;
    box_sweep(pa, valid, D.bbox, D.nbox, 0, D.nbox, D.b, D.nb, d2_thres, lx, ly, lz, [&](int j, const float (&pb)[3], float d2) {
        const float4 blo4 = ld4s(D.b + lo_off(j)), bhi4 = ld4s(D.b + hi_off(D.nb, j));
        const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
        const float d2c = pair_d2c(fa, fb);
        if (!(d2c < d2c_thres)) return;                                      // cvo.cpp:428
        const float a = pair_ck(d2c, csig2, den_c) * pair_k(d2, sig2, den_l);    // cvo.cpp:429-431
        sumA += a; count += 1;                                               // cvo.cpp:432-435, this row's terms in ascending columns
    });

    double cnt = (double)count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sumA += __shfl_xor(sumA, off, 64);
    if (tid < 2) partials[rec * 2 + tid] = tid == 0 ? sumA : cnt;
}

// One wave per pair.  scores: pairs x K records and best: one int per pair, both in pinned host memory (no copy engine, as cvo_score_reduce_kernel);
// seed != 0: lane 0 also writes the pair's device-resident start state -- every word zero, R and T from reset_initial(hypothesis[best]) on a fresh
// object (transform = I: keyframe_graph.cpp:696, cvo.cpp:611-618; reset_initial_eval is the function cvo_track_link_kernel and the host's
// cvo_reset_initial call), ell, transform and iter as the pair's start state carries them.
__global__ __launch_bounds__(HYP_BLOCK) void cvo_hyp_reduce_select_kernel(const HypDesc* __restrict__ descs, const double* __restrict__ partials, int K, int row_blocks,
                                                                           HypScore* __restrict__ scores, int* __restrict__ best, int seed) {
    const int p = blockIdx.x, k = threadIdx.x;
    float value = -__builtin_inff(); int idx = HYP_MAX;              // a lane without a hypothesis never wins: every value is a sum of positive terms
    if (k < K) {
        const double* r = partials + ((size_t)p * K + k) * (size_t)row_blocks * 2;
        double sum = 0, cnt = 0;
#pragma unroll 4
        for (int blk = 0; blk < row_blocks; ++blk) { sum += r[2 * blk]; cnt += r[2 * blk + 1]; }   // ascending blocks
        if (cnt == 0) cnt = 1;                                       // cvo.cpp:455-456
        HypScore o; o.value = (float)sum; o.num = (int)cnt; o.num_e = 0;   // cvo.cpp:457
        scores[(size_t)p * K + k] = o;
        value = o.value; idx = k;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                         // the largest f32 value, its lowest index
        const float ov = __shfl_xor(value, off, 64); const int oi = __shfl_xor(idx, off, 64);
        if (ov > value || (ov == value && oi < idx)) { value = ov; idx = oi; }
    }
    if (k != 0) return;                                              // (lane 0 holds a hypothesis, K >= 1: its idx is below K whatever the values are)
    best[p] = idx;
    if (!seed) return;
    const HypDesc& D = descs[p];
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float hyp[12], R[9], T[3], inv[12];
    for (int q = 0; q < 12; ++q) hyp[q] = D.trans[12 * (size_t)idx + q];
    reset_initial_eval(I, hyp, R, T, inv);
    PairState* st = D.state;
    unsigned* w = reinterpret_cast<unsigned*>(st);
    for (unsigned q = 0; q < sizeof(PairState) / sizeof(unsigned); ++q) w[q] = 0u;
    for (int q = 0; q < 9; ++q) st->R[q] = R[q];
    for (int q = 0; q < 3; ++q) st->T[q] = T[q];
    st->ell = D.seed_ell;
    for (int q = 0; q < 12; ++q) st->transform[q] = D.seed_transform[q];
    st->iter = D.seed_iter;
}

int hyp_row_blocks(int na) { return (na + HYP_BLOCK - 1) / HYP_BLOCK; }
int hyp_max() { return HYP_MAX; }

// One call's two launches on `stream`: the sweep over (row_blocks, k, n_pairs) workgroups, then the reduce / select step.  descs: n_pairs
// descriptors in device memory; partials: n_pairs * k * row_blocks records of two doubles; scores, best: device-readable pinned host memory.
hipError_t launch_hypotheses(const HypDesc* descs, int n_pairs, int k, int row_blocks, const DevParams& P, double* partials, HypScore* scores, int* best,
                             int seed, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    hipLaunchKernelGGL(cvo_hyp_score_kernel, dim3(row_blocks, k, n_pairs), dim3(HYP_BLOCK), 0, stream, descs, P, partials, wgs_started);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sweep_submitted) *sweep_submitted = true;                   // its workgroups will count themselves as started
    hipLaunchKernelGGL(cvo_hyp_reduce_select_kernel, dim3(n_pairs), dim3(HYP_BLOCK), 0, stream, descs, partials, k, row_blocks, scores, best, seed);
    return hipGetLastError();
}

}  // namespace cvohip
