// cvo_sweep.hpp -- what cvo_score_kernel (cvo_score_kernels.hip), cvo_support_kernel (cvo_support_kernels.hip) and the align launch's
// tail scores (cvo_kernels.hip, score_pair_terms) have in common, written once: the group boxes of a cloud, the box-culled radius sweep
// of 64 rows over a cloud's columns, and the reference's arithmetic of one pair.  The tests hold these three places to the same bits.
// cvo_hyp_score_kernel (cvo_hypothesis_kernels.hip) and cvo_pose_model_sweep_kernel (cvo_pose_model_kernels.hip) are built on the same pieces.
//
// The sweep.  The radius search the reference runs per point (KD-tree, nanoflann) is restated as a box cull: clouds come in image scan
// order, so 32 consecutive points span the image width but only a few image rows -- every cloud carries the bounding boxes of its
// 32-point groups (x, y, z and the ray slope y/z; store_group_box), a wave (workgroup = one wave = 64 rows, lane = row) tests its own
// rows' box against 64 group boxes at a time (one ballot), and only the groups that can hold a neighbour (a few percent at the radii in
// use) are staged in LDS, SWEEP_STAGE at a time (their loads overlap; every lane then reads the same 16 bytes: a broadcast), and swept
// with a fused test whose sign bits are collected in a 32-bit word.  The radius gate IS binding here (no a > sp_thres test, Q6), so a
// hit of the fused sweep is re-tested with the reference's own un-fused d2 expression (nanoflann.hpp:403-406) before it counts.  Rows
// see their columns in ascending order, as in the reference's sorted radius search.  Arbitrarily ordered clouds stay correct: their
// boxes are just loose.
//
// Every constant carries a guarantee.  thr_cull = d2_thres (1 + 1e-6) covers the fused test's rounding against the un-fused one;
// thr_box = thr_cull * 1.001 and the slope bound's 1.01 and 1.0e-6f cover the box gaps' rounding: a skipped group holds no hit.  A
// point at or behind the camera (z <= 1.0e-3f) has no slope bound.  Padding rows sit at +3.0e18f and padding columns at -3.0e18f:
// finite squares, far outside every radius.  Compiled with -ffp-contract=off: the source order is the rounding order, and the FMAs
// asked for below are the only ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cvo_device.h"
#include "cvo_math.hpp"

namespace cvohip {

constexpr int SWEEP_STAGE = 4;     // near groups fetched per round; the callers' three LDS arrays hold 32 * SWEEP_STAGE floats each

__device__ __forceinline__ float4 ld4s(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float wmin(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// The box of one 32-point group of the {x, y, z, f0} plane rec (n points): a wave of 64 lanes makes groups 2 * blockIdx.x and
// 2 * blockIdx.x + 1, lane & 31 = point of the group.  gbox: planes lo x, y, z, slope then hi x, y, z, slope, ngroups floats each.
__device__ __forceinline__ void store_group_box(const float* __restrict__ rec, int n, float* __restrict__ gbox, int ngroups) {
    const int lane = threadIdx.x, gi = blockIdx.x * 2 + (lane >> 5), j = gi * 32 + (lane & 31);
    const float INF = __builtin_inff();
    float lo[4] = {INF, INF, INF, INF}, hi[4] = {-INF, -INF, -INF, -INF};
    if (j < n) {
        const float4 p = ld4s(rec + lo_off(j));
        lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
        if (p.z > 1.0e-3f) { lo[3] = hi[3] = p.y / p.z; } else { lo[3] = -INF; hi[3] = INF; }   // behind / at the camera: no slope bound
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { lo[q] = fminf(lo[q], __shfl_xor(lo[q], off, 64)); hi[q] = fmaxf(hi[q], __shfl_xor(hi[q], off, 64)); }
    }
    if ((lane & 31) == 0 && gi < ngroups) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { gbox[q * ngroups + gi] = lo[q]; gbox[(4 + q) * ngroups + gi] = hi[q]; }
    }
}

// One wave's rows against the column groups [g_begin, g_end) of a cloud: hit(j, pb, d2) for every column j (point pb) with the
// reference's un-fused d2 < d2_thres (cvo.cpp:423 / 654), columns ascending.  pa: this lane's row (anything when !valid: such a lane
// is kept out of the wave's box and should hold the padding point); bbox, ngroups: the columns' boxes; b_lo, nb: their {x, y, z, f0}
// plane; lx, ly, lz: 32 * SWEEP_STAGE floats of LDS each, 16-byte aligned.  Called by all 64 lanes (it holds barriers); an empty
// range returns at once.
template <class Hit>
__device__ __forceinline__ void box_sweep(const float (&pa)[3], bool valid, const float* __restrict__ bbox, int ngroups, int g_begin, int g_end,
                                          const float* __restrict__ b_lo, int nb, float d2_thres, float* lx, float* ly, float* lz, Hit&& hit) {
    const int tid = threadIdx.x;
    const float thr_cull = d2_thres * (1.0f + 1e-6f);
    const float thr_box = thr_cull * 1.001f;                                     // box gaps are compared with a margin: a skipped group holds no hit
    const float Rb = sqrtf(fmaxf(thr_cull, 0.f));
    const float INF = __builtin_inff();
    float blo[4] = {INF, INF, INF, INF}, bhi[4] = {-INF, -INF, -INF, -INF};
    if (valid) {
#pragma unroll
        for (int q = 0; q < 3; ++q) blo[q] = bhi[q] = pa[q];
        if (pa[2] > 1.0e-3f) { blo[3] = bhi[3] = pa[1] / pa[2]; } else { blo[3] = -INF; bhi[3] = INF; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { blo[q] = wmin(blo[q]); bhi[q] = wmax(bhi[q]); }
    // points p (a row), q (a column) within Rb of each other: |y_p/z_p - y_q/z_q| <= Rb (1 + |y_q/z_q|) / z_p
    const float slope_reach = (blo[2] > 1.0e-3f) ? Rb * 1.01f / blo[2] : INF;
    const float nthr = -thr_cull;

    for (int gb = g_begin; gb < g_end; gb += 64) {
        bool near = false;
        if (gb + tid < g_end) {
            float gap2 = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float glo = bbox[q * ngroups + gb + tid], ghi = bbox[(4 + q) * ngroups + gb + tid];
                const float d = fmaxf(0.f, fmaxf(glo - bhi[q], blo[q] - ghi));
                gap2 = __builtin_fmaf(d, d, gap2);
            }
            const float tlo = bbox[3 * ngroups + gb + tid], thi = bbox[7 * ngroups + gb + tid];
            const float tgap = fmaxf(0.f, fmaxf(tlo - bhi[3], blo[3] - thi));
            const float tabs = fmaxf(fabsf(tlo), fabsf(thi));
            near = (gap2 <= thr_box) && (tgap <= slope_reach * (1.0f + tabs) + 1.0e-6f);   // false for NaN (inf - inf)
        }
        unsigned long long mask = __ballot(near);
        while (mask) {
            // up to SWEEP_STAGE near groups are fetched together (their loads overlap), then swept one after the other
            int gis[SWEEP_STAGE]; int ns = 0;
#pragma unroll
            for (int k = 0; k < SWEEP_STAGE; ++k) {
                gis[k] = -1;
                if (mask) { gis[k] = gb + __builtin_ctzll(mask); mask &= mask - 1ull; ns = k + 1; }
            }
            __syncthreads();                                        // the previous groups have been swept
#pragma unroll
            for (int pass = 0; pass < SWEEP_STAGE / 2; ++pass) {
                const int gsel = (tid >> 5) ? gis[2 * pass + 1] : gis[2 * pass];
                if (gsel >= 0) {
                    const int j = gsel * 32 + (tid & 31);
                    float b0 = -3.0e18f, b1 = -3.0e18f, b2 = -3.0e18f;
                    if (j < nb) { const float4 lo = ld4s(b_lo + lo_off(j)); b0 = lo.x; b1 = lo.y; b2 = lo.z; }
                    lx[pass * 64 + tid] = b0; ly[pass * 64 + tid] = b1; lz[pass * 64 + tid] = b2;
                }
            }
            __syncthreads();
            for (int k = 0; k < ns; ++k) {
                int gi = gis[0];
#pragma unroll
                for (int k2 = 1; k2 < SWEEP_STAGE; ++k2) gi = (k == k2) ? gis[k2] : gi;
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
                    if (!(d2 < d2_thres)) continue;                                      // cvo.cpp:423 / 654
                    hit(j, pb, d2);
                }
            }
        }
    }
}

// ---- One pair (row point pa with features fa, column point pb with features fb) as the reference computes it.
// colour gate: d2c, to be held against d2c_thres (cvo.cpp:428 / 659)
__device__ __forceinline__ float pair_d2c(const float (&fa)[5], const float (&fb)[5]) {
    float t[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) { const float e = fa[c] - fb[c]; t[c] = e * e; }
    return (t[0] + t[1]) + (t[2] + (t[3] + t[4]));
}
// sig2 = sigma^2, den_l = 2 ell^2 (cvo.cpp:429 / 661); csig2 = c_sigma^2, den_c = 2 c_ell^2 (cvo.cpp:430): double exp, the division as written
__device__ __forceinline__ float pair_k(float d2, float sig2, double den_l) { return (float)((double)sig2 * exp((double)(-d2) / den_l)); }
__device__ __forceinline__ float pair_ck(float d2c, float csig2, double den_c) { return (float)((double)csig2 * exp((double)(-d2c) / den_c)); }
// se3_Hessian's 21 terms of the pair (cvo.cpp:665-704), each a float, times the float weight wgt, each product a float, added to H; il2 = 1 / ell^2.
// Acc: float as the reference keeps its Hessian (cvo.cpp:622, 707), or double (cvo_pose_model_kernels.hip).  cr = pa x pb and db = pb - pa are
// handed back: the gradient's terms are made of them.
template <class Acc>
__device__ __forceinline__ void pair_hessian_add_weighted(const float (&pa)[3], const float (&pb)[3], float il2, float wgt, Acc (&H)[21], float (&cr)[3], float (&db)[3]) {
    cross3(pa, pb, cr);
    const float dot1 = pa[1] * pb[1] + pa[2] * pb[2], dot2 = pa[0] * pb[0] + pa[2] * pb[2], dot3 = pa[0] * pb[0] + pa[1] * pb[1];
    db[0] = pb[0] - pa[0]; db[1] = pb[1] - pa[1]; db[2] = pb[2] - pa[2];
    float Bq[21];
    // block A (symmetric): 00 01 02 11 12 22                          cvo.cpp:670-675
    Bq[0] = il2 * cr[0] * cr[0] - dot1;
    Bq[1] = (float)(il2 * cr[0] * cr[1] + 0.5 * (pa[0] * pb[1] + pa[1] * pb[0]));
    Bq[2] = (float)(il2 * cr[0] * cr[2] + 0.5 * (pa[0] * pb[2] + pa[2] * pb[0]));
    Bq[3] = il2 * cr[1] * cr[1] - dot2;
    Bq[4] = (float)(il2 * cr[1] * cr[2] + 0.5 * (pa[1] * pb[2] + pa[2] * pb[1]));
    Bq[5] = il2 * cr[2] * cr[2] - dot3;
    // block C (full 3x3, row-major C(r,c))                            cvo.cpp:680-688
    Bq[6] = il2 * cr[0] * db[0];          Bq[7] = -pa[2] + il2 * db[0] * cr[1];  Bq[8] = pa[1] + il2 * db[0] * cr[2];
    Bq[9] = pa[2] + il2 * db[1] * cr[0];  Bq[10] = il2 * cr[1] * db[1];          Bq[11] = -pa[0] + il2 * db[1] * cr[2];
    Bq[12] = -pa[1] + il2 * db[2] * cr[0]; Bq[13] = pa[0] + il2 * db[2] * cr[1]; Bq[14] = il2 * cr[2] * db[2];
    // block D (symmetric): 00 01 02 11 12 22                          cvo.cpp:692-697
    Bq[15] = il2 * db[0] * db[0] - 1; Bq[16] = il2 * db[0] * db[1]; Bq[17] = il2 * db[0] * db[2];
    Bq[18] = il2 * db[1] * db[1] - 1; Bq[19] = il2 * db[1] * db[2]; Bq[20] = il2 * db[2] * db[2] - 1;
#pragma unroll
    for (int q2 = 0; q2 < 21; ++q2) H[q2] += wgt * Bq[q2];
}
// the reference's weight: the features' dot product where the energy has ck (cvo.cpp:662, 707)
__device__ __forceinline__ void pair_hessian_add(const float (&pa)[3], const float (&fa)[5], const float (&pb)[3], const float (&fb)[5], float il2, float k, float (&H)[21]) {
    float t[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) t[c] = fa[c] * fb[c];
    const float cdot = (t[0] + t[1]) + (t[2] + (t[3] + t[4]));       // cvo.cpp:662
    float cr[3], db[3];
    pair_hessian_add_weighted(pa, pb, il2, il2 * cdot * k, H, cr, db);   // cvo.cpp:707
}

}  // namespace cvohip
