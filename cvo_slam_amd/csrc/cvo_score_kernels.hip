// cvo_score_kernels.hip -- function_inner_product (cvo.cpp:388-459) and
// se3_Hessian (cvo.cpp:620-759) as one all-pairs kernel; a whole score block
// (compute_innerproduct: 4 inner products + 1 Hessian, cvo.cpp:475-503; the loop-closure
// variant: 6 + 2, cvo.cpp:505-561; a batch of either) is ONE launch.
//
// Grid = (64-row blocks of cloud a) x (column chunks of cloud b) x (requests).  Workgroup =
// one wave, thread = one point of cloud a (optionally transformed first, cvo.cpp:485-487).
// The radius search is the box-culled sweep of cvo_sweep.hpp (box_sweep) over this
// workgroup's chunk of the columns' groups, the pair arithmetic that header's too.  What
// this kernel adds: the column chunks, the shortcut for a cached self inner product, and
// the sums -- per-thread sums are f32 for the Hessian (the reference keeps an f32 Hessian,
// cvo.cpp:622,707), f64 across threads; every workgroup writes one partial record
// and a second tiny kernel adds the records of a request in a fixed order straight into
// pinned host memory, so results are reproducible run to run and no copy engine is
// involved.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"
#include "cvo_sweep.hpp"

namespace cvohip {

constexpr int SCORE_BLOCK = 64;
constexpr int SCORE_NOUT = 24;     // sum_A, count, 21 Hessian terms, pad

// boxes of a cloud's 32-point groups: planes lo x, y, z, slope then hi x, y, z, slope, ngroups floats each; behind them the cloud's
// table of cached self inner products (ScoreDesc::self_cache), emptied here: the boxes are remade whenever the points were written
__global__ __launch_bounds__(64) void cvo_cloud_boxes_kernel(const float* __restrict__ rec, int n, float* __restrict__ gbox, int ngroups, SelfCacheEntry* __restrict__ self_cache) {
    if (blockIdx.x == 0 && threadIdx.x < SELF_CACHE_N) { SelfCacheEntry e; e.ell = 0.f; e.valid = 0; e.sum = 0.0; e.count = 0.0; self_cache[threadIdx.x] = e; }
    store_group_box(rec, n, gbox, ngroups);
}

// The same boxes for MANY clouds in one launch (the frames staged ahead of a K-stream step: cvo_batch_stage_images, cvo_tracks_stage_async):
// grid.y = cloud, grid.x = pairs of groups of the largest cloud; a workgroup (one wave) past its cloud's last group leaves at once.
__global__ __launch_bounds__(64) void cvo_cloud_boxes_batch_kernel(const BoxDesc* __restrict__ descs) {
    const BoxDesc D = descs[blockIdx.y];
    if ((int)blockIdx.x * 2 >= D.ngroups) return;                     // (uniform over the wave; ngroups >= 1, so block 0 of every cloud stays)
    if (blockIdx.x == 0 && threadIdx.x < SELF_CACHE_N) { SelfCacheEntry e; e.ell = 0.f; e.valid = 0; e.sum = 0.0; e.count = 0.0; D.self_cache[threadIdx.x] = e; }
    store_group_box(D.rec, D.n, D.gbox, D.ngroups);
}

__global__ __launch_bounds__(SCORE_BLOCK) void cvo_score_kernel(ScoreBatch B, const ScoreDesc* __restrict__ more, DevParams P, double* __restrict__ partials,
                                                                unsigned* __restrict__ wgs_started) {
    // adoption's "is anything queued on the device?" (cvo_capi.hip, AdoptCounters): this workgroup has started
    if (wgs_started && threadIdx.x == 0) atomicAdd(wgs_started, 1u);
    const ScoreDesc& D = more ? more[blockIdx.z] : B.d[blockIdx.z];     // a tracker's score block travels in the kernel arguments, a batch's in HBM
    __shared__ __attribute__((aligned(16))) float lx[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float ly[32 * SWEEP_STAGE];
    __shared__ __attribute__((aligned(16))) float lz[32 * SWEEP_STAGE];

    const int tid = threadIdx.x, i = blockIdx.x * SCORE_BLOCK + tid;
    const float ell = D.from ? D.from->ell : D.ell, sigma = P.sigma;
    if (D.self_cache) {
        // fip(cloud, cloud) at this ell is already known (cvo.cpp:496-497 depend on the cloud and ell alone): the request's first record
        // carries the cached sums, the others zeros, and the reduction below adds them up to the very same doubles.  Every workgroup of
        // the launch sees the same table: it is written by the reduce kernel only, and launches that touch a cloud are ordered (ensure_boxes).
        int hit = -1;
#pragma unroll
        for (int e = 0; e < SELF_CACHE_N; ++e) if (D.self_cache[e].valid && D.self_cache[e].ell == ell) hit = e;
        if (hit >= 0) {
            const size_t rec0 = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            const bool first = blockIdx.x == 0 && blockIdx.y == 0;
            if (tid < SCORE_NOUT) partials[rec0 * SCORE_NOUT + tid] = (first && tid == 0) ? D.self_cache[hit].sum : ((first && tid == 1) ? D.self_cache[hit].count : 0.0);
            return;
        }
    }
    const float d2_thres = gate_d2_score(ell, P.sp_thres, sigma);                // cvo.cpp:395 / 626
    const float d2c_thres = gate_d2c(P.c_ell, P.sp_thres, P.c_sigma);            // cvo.cpp:396 / 627
    const double den_l = 2.0 * ell * ell, den_c = 2.0 * P.c_ell * P.c_ell;
    const float sig2 = sigma * sigma, csig2 = P.c_sigma * P.c_sigma;
    const float il2 = 1 / (ell * ell);

    float pa[3] = {3.0e18f, 3.0e18f, 3.0e18f};
    float fa[5] = {0, 0, 0, 0, 0};
    const bool valid = i < D.na;
    if (valid) {
        const float4 lo = ld4s(D.a + lo_off(i)), hi = ld4s(D.a + hi_off(D.na, i));
        if (D.use_tran) apply_transform(D.use_tran == 2 ? D.from->transform : D.tran, lo.x, lo.y, lo.z, pa[0], pa[1], pa[2]);
        else { pa[0] = lo.x; pa[1] = lo.y; pa[2] = lo.z; }
        fa[0] = lo.w; fa[1] = hi.x; fa[2] = hi.y; fa[3] = hi.z; fa[4] = hi.w;
    }

    double sumA = 0; int count = 0;
    float H[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) H[q] = 0.f;

    // this workgroup's chunk of cloud b, in 32-point groups; none for a row block past the end of the request's cloud
    const int ngroups = D.nbox;
    const int gper = (ngroups + (int)gridDim.y - 1) / (int)gridDim.y;
    const int g_begin = min(ngroups, (int)blockIdx.y * gper), g_end = min(ngroups, g_begin + gper);
    const bool any_row = blockIdx.x * SCORE_BLOCK < D.na;
    box_sweep(pa, valid, D.bbox, ngroups, g_begin, any_row ? g_end : g_begin, D.b, D.nb, d2_thres, lx, ly, lz, [&](int j, const float (&pb)[3], float d2) {
        const float4 blo4 = ld4s(D.b + lo_off(j)), bhi4 = ld4s(D.b + hi_off(D.nb, j));
        const float fb[5] = {blo4.w, bhi4.x, bhi4.y, bhi4.z, bhi4.w};
        const float d2c = pair_d2c(fa, fb);
        if (!(d2c < d2c_thres)) return;                                      // cvo.cpp:428 / 659
        const float k = pair_k(d2, sig2, den_l);                             // cvo.cpp:429 / 661
        if (!D.want_hessian) {
            const float a = pair_ck(d2c, csig2, den_c) * k;                  // cvo.cpp:430-431
            sumA += a; count += 1;                                           // cvo.cpp:432-435
        } else {
            pair_hessian_add(pa, fa, pb, fb, il2, k, H);
            count += 1;
        }
    });

    const size_t rec = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    double cnt = (double)count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (!D.want_hessian) {                                          // inner product: two sums
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sumA += __shfl_xor(sumA, off, 64);
        if (tid < SCORE_NOUT) partials[rec * SCORE_NOUT + tid] = tid == 0 ? sumA : (tid == 1 ? cnt : 0.0);   // row blocks past the end of a request's cloud write zeros
        return;
    }
    double mine = tid == 1 ? cnt : 0.0;
#pragma unroll
    for (int q = 0; q < 21; ++q) {
        double t = (double)H[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        mine = (tid == 2 + q) ? t : mine;
    }
    if (tid < SCORE_NOUT) partials[rec * SCORE_NOUT + tid] = mine;
}

// one workgroup per request: its partial records into out[request][24] (pinned host memory).  Eight lanes per output walk
// the records r = part, part + 8, ... in order, then the eight partial sums are added in lane order: a fixed order, so the
// result does not depend on timing.
__global__ __launch_bounds__(256) void cvo_score_reduce_kernel(ScoreBatch B, const ScoreDesc* __restrict__ more, const double* __restrict__ partials, int records_per_request, double* __restrict__ out) {
    __shared__ double part_sum[8][32];
    __shared__ double totals[SCORE_NOUT];
    const int tid = threadIdx.x, q = tid & 31, part = tid >> 5;
    const double* p = partials + (size_t)blockIdx.x * records_per_request * SCORE_NOUT;
    double s = 0;
    if (q < SCORE_NOUT) for (int r = part; r < records_per_request; r += 8) s += p[(size_t)r * SCORE_NOUT + q];
    part_sum[part][q] = s;
    __syncthreads();
    if (tid < SCORE_NOUT) {
        double t = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += part_sum[k][tid];
        out[blockIdx.x * SCORE_NOUT + tid] = t;
        totals[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {                                                 // a self inner product that was computed: keep it with the cloud
        const ScoreDesc& D = more ? more[blockIdx.x] : B.d[blockIdx.x];
        if (D.self_cache) {
            const float ell = D.from ? D.from->ell : D.ell;
            int at = -1, free_at = -1;
            for (int e = 0; e < SELF_CACHE_N; ++e) {
                if (D.self_cache[e].valid && D.self_cache[e].ell == ell) at = e;
                if (!D.self_cache[e].valid && free_at < 0) free_at = e;
            }
            if (at < 0) {
                SelfCacheEntry ne; ne.ell = ell; ne.valid = 1; ne.sum = totals[0]; ne.count = totals[1];
                D.self_cache[free_at >= 0 ? free_at : SELF_CACHE_N - 1] = ne;
            }
        }
    }
}

int score_nout() { return SCORE_NOUT; }
int score_groups(int n) { return (n + 31) / 32; }
static size_t score_box_floats(int n) { return (8 * (size_t)score_groups(n) + 3) & ~(size_t)3; }   // the table behind the boxes starts 16-byte aligned
size_t score_box_bytes(int n) { return sizeof(float) * score_box_floats(n) + sizeof(SelfCacheEntry) * SELF_CACHE_N; }
SelfCacheEntry* score_self_cache(float* gbox, int n) { return reinterpret_cast<SelfCacheEntry*>(gbox + score_box_floats(n)); }
hipError_t launch_cloud_boxes(const float* rec, int n, float* gbox, hipStream_t stream) {
    const int ng = score_groups(n);
    hipLaunchKernelGGL(cvo_cloud_boxes_kernel, dim3((ng + 1) / 2), dim3(64), 0, stream, rec, n, gbox, ng, score_self_cache(gbox, n));
    return hipGetLastError();
}
// descs: n_clouds descriptors the device can read (pinned host memory), every cloud with n > 0; n_max: the largest n among them
hipError_t launch_cloud_boxes_batch(const BoxDesc* descs, int n_clouds, int n_max, hipStream_t stream) {
    if (n_clouds <= 0 || n_max <= 0) return hipSuccess;
    hipLaunchKernelGGL(cvo_cloud_boxes_batch_kernel, dim3((score_groups(n_max) + 1) / 2, n_clouds), dim3(64), 0, stream, descs);
    return hipGetLastError();
}
int score_row_blocks(int na) { return (na + SCORE_BLOCK - 1) / SCORE_BLOCK; }

// one launch for the whole batch of requests; out_pinned[request][24] is complete when the stream has drained
hipError_t launch_score(const ScoreBatch& B, const ScoreDesc* more, int nreq, int row_blocks, int chunks, const DevParams& P, double* partials,
                        double* out_pinned, hipStream_t stream, unsigned* wgs_started, bool* sweep_submitted) {
    if (sweep_submitted) *sweep_submitted = false;
    hipLaunchKernelGGL(cvo_score_kernel, dim3(row_blocks, chunks, nreq), dim3(SCORE_BLOCK), 0, stream, B, more, P, partials, wgs_started);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sweep_submitted) *sweep_submitted = true;                   // its workgroups will count themselves as started
    hipLaunchKernelGGL(cvo_score_reduce_kernel, dim3(nreq), dim3(256), 0, stream, B, more, partials, row_blocks * chunks, out_pinned);
    return hipGetLastError();
}

}  // namespace cvohip
