// cvo_eigen337.hpp -- the two epilogue pieces of the "Eigen 3.3.7" arithmetic mode (include/cvo_hip.h: CVO_ARITH_*), written once for
// the device epilogue (one lane per workgroup), the self-test kernels and a plain host build (tests/test_arith_mode_host.py compiles this
// header alone with g++ -ffp-contract=off).
//
//   cubic_step_f32eig  poly_solver + root selection as the reference runs them (cvo.cpp:76-92, 324-333): the f32 companion matrix of the
//                      monic step cubic, its eigenvalues by f32 Householder Hessenberg reduction + Francis double-shift QR (the EISPACK hqr
//                      scheme behind Eigen's RealSchur), the smallest positive one with a zero imaginary part, min_step if there is none,
//                      clamped to 0.8.
//   dist_se3_f32logm   dist_se3 as the reference runs it (cvo.cpp:94-104): the Frobenius norm of Matrix4f::log() of [dR dT; 0 1], by inverse
//                      scaling and squaring on the f32 real Schur form (Denman-Beavers square roots, Gauss-Legendre partial-fraction Pade of
//                      degree 3..5 with the single-precision thresholds of Eigen's MatrixLogarithm.h).
//
// These are the published algorithms in f32, the same reading the test oracle's reference-noise variants make (ORC_VAR_F32_ROOTS,
// ORC_VAR_F32_LOGM): same operations in the same order, so the same bits as that reading -- but not Eigen's own bits, which no build
// here has pinned.  Only + - * /, sqrtf, fabsf, ldexpf and isfinite; every float expression rounds as written (-ffp-contract=off).
// The double constants below are rounded to f32 once, as the oracle rounds them.
#pragma once
#include <math.h>

#ifndef CVO_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define CVO_HD __host__ __device__ __forceinline__
#else
#define CVO_HD inline
#endif
#endif

namespace cvohip {
namespace e337 {

constexpr float FLT_EPS = 1.1920928955078125e-7f;   // std::numeric_limits<float>::epsilon()

struct M4 { float a[4][4]; };

CVO_HD void m4_identity(M4& m) { for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m.a[i][j] = (i == j) ? 1.f : 0.f; }
CVO_HD float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max

CVO_HD void m4_mul(const M4& A, const M4& B, int n, M4& C) {
    m4_identity(C);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { float s = 0.f; for (int k = 0; k < n; ++k) s += A.a[i][k] * B.a[k][j]; C.a[i][j] = s; }
}

// H <- P H P, U <- U P for the Householder reflector P = I - beta v v^T on rows / columns r0 .. r0+len-1
CVO_HD void apply_reflector(M4& H, M4& U, int n, int r0, int len, const float* v, float beta) {
    for (int c = 0; c < n; ++c) {
        float s = 0.f; for (int k = 0; k < len; ++k) s += v[k] * H.a[r0 + k][c];
        s *= beta; for (int k = 0; k < len; ++k) H.a[r0 + k][c] -= s * v[k];
    }
    for (int r = 0; r < n; ++r) {
        float s = 0.f; for (int k = 0; k < len; ++k) s += H.a[r][r0 + k] * v[k];
        s *= beta; for (int k = 0; k < len; ++k) H.a[r][r0 + k] -= s * v[k];
        float t = 0.f; for (int k = 0; k < len; ++k) t += U.a[r][r0 + k] * v[k];
        t *= beta; for (int k = 0; k < len; ++k) U.a[r][r0 + k] -= t * v[k];
    }
}
// v, beta with (I - beta v v^T) x = -/+ |x| e1; false when x is zero beyond its first entry
CVO_HD bool make_reflector(const float* x, int len, float* v, float& beta) {
    float tail = 0.f; for (int k = 1; k < len; ++k) tail += x[k] * x[k];
    if (tail == 0.f) return false;
    const float nrm = sqrtf(x[0] * x[0] + tail);
    const float alpha = (x[0] >= 0) ? -nrm : nrm;
    v[0] = x[0] - alpha; for (int k = 1; k < len; ++k) v[k] = x[k];
    float vv = 0.f; for (int k = 0; k < len; ++k) vv += v[k] * v[k];
    beta = 2.f / vv;
    return true;
}

// real Schur form A = U T U^T of the leading n x n block; false if the QR iteration does not converge (60 n sweeps)
CVO_HD bool real_schur(M4& T, M4& U, int n) {
    m4_identity(U);
    for (int k = 0; k + 2 < n; ++k) {                                   // Householder Hessenberg reduction
        float x[4], v[4], beta;
        const int len = n - k - 1;
        for (int i = 0; i < len; ++i) x[i] = T.a[k + 1 + i][k];
        if (make_reflector(x, len, v, beta)) {
            apply_reflector(T, U, n, k + 1, len, v, beta);
            for (int i = k + 2; i < n; ++i) T.a[i][k] = 0.f;
        }
    }
    float norm = 0.f; for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) norm += fabsf(T.a[i][j]);
    int hi = n - 1, iter = 0, total = 0;
    while (hi > 0) {
        int l = hi;
        while (l > 0) {                                                 // deflation test
            float s = fabsf(T.a[l - 1][l - 1]) + fabsf(T.a[l][l]);
            if (s == 0.f) s = norm;
            if (fabsf(T.a[l][l - 1]) <= FLT_EPS * s) { T.a[l][l - 1] = 0.f; break; }
            --l;
        }
        if (l == hi) { --hi; iter = 0; continue; }
        if (l == hi - 1) {                                              // 2x2 block: split it when its eigenvalues are real
            const float a = T.a[hi - 1][hi - 1], b = T.a[hi - 1][hi], c = T.a[hi][hi - 1], d = T.a[hi][hi];
            const float p = 0.5f * (a - d), q = p * p + b * c;
            if (q >= 0) {
                const float z = sqrtf(q);
                const float w = (p >= 0) ? p + z : p - z;
                const float r = sqrtf(w * w + c * c);
                const float cs = w / r, sn = c / r;
                for (int col = 0; col < n; ++col) {
                    const float t0 = T.a[hi - 1][col], t1 = T.a[hi][col];
                    T.a[hi - 1][col] = cs * t0 + sn * t1; T.a[hi][col] = -sn * t0 + cs * t1;
                }
                for (int row = 0; row < n; ++row) {
                    const float t0 = T.a[row][hi - 1], t1 = T.a[row][hi];
                    T.a[row][hi - 1] = cs * t0 + sn * t1; T.a[row][hi] = -sn * t0 + cs * t1;
                    const float u0 = U.a[row][hi - 1], u1 = U.a[row][hi];
                    U.a[row][hi - 1] = cs * u0 + sn * u1; U.a[row][hi] = -sn * u0 + cs * u1;
                }
                T.a[hi][hi - 1] = 0.f;
            }
            hi -= 2; iter = 0; continue;
        }
        if (++total > 60 * n) return false;
        // Francis double-shift step on the active block l .. hi (EISPACK hqr: the shift polynomial's first column from differences)
        float xx = T.a[hi][hi], yy = T.a[hi - 1][hi - 1], w = T.a[hi][hi - 1] * T.a[hi - 1][hi];
        if (iter == 10 || iter == 30) {                                 // exceptional shift
            const float e = fabsf(T.a[hi][hi - 1]) + fabsf(T.a[hi - 1][hi - 2]);
            xx = yy = xx + 0.75f * e; w = -0.4375f * e * e;
        }
        ++iter;
        int m = hi - 2;
        float p = 0.f, q = 0.f, r = 0.f;
        for (;; --m) {
            const float zz = T.a[m][m], rr = xx - zz, ss = yy - zz;
            p = (rr * ss - w) / T.a[m + 1][m] + T.a[m][m + 1];
            q = T.a[m + 1][m + 1] - zz - rr - ss;
            r = T.a[m + 2][m + 1];
            const float sc = fabsf(p) + fabsf(q) + fabsf(r);
            if (sc != 0.f) { p /= sc; q /= sc; r /= sc; }
            if (m == l) break;
            const float lhs = fabsf(T.a[m][m - 1]) * (fabsf(q) + fabsf(r));
            const float rhs = fabsf(p) * (fabsf(T.a[m - 1][m - 1]) + fabsf(zz) + fabsf(T.a[m + 1][m + 1]));
            if (lhs <= FLT_EPS * rhs) break;
        }
        for (int k = m; k <= hi - 1; ++k) {
            const int len = (k == hi - 1) ? 2 : 3;
            float xv[3], v[3], beta;
            if (k == m) { xv[0] = p; xv[1] = q; xv[2] = r; }
            else { xv[0] = T.a[k][k - 1]; xv[1] = T.a[k + 1][k - 1]; xv[2] = (len == 3) ? T.a[k + 2][k - 1] : 0.f; }
            if (!make_reflector(xv, len, v, beta)) continue;
            if (k == m && m > l) {                                      // the negligible T[m][m-1] only changes sign
                const float keep = T.a[m][m - 1];
                T.a[m][m - 1] = 0.f;
                apply_reflector(T, U, n, k, len, v, beta);
                T.a[m][m - 1] = -keep;
            } else {
                apply_reflector(T, U, n, k, len, v, beta);
            }
            if (k > m) { T.a[k + 1][k - 1] = 0.f; if (len == 3) T.a[k + 2][k - 1] = 0.f; }
        }
    }
    return true;
}

// eigenvalues of the leading n x n block; real ones carry im == 0 exactly
CVO_HD bool eigenvalues(const M4& A, int n, float* re, float* im) {
    M4 T = A, U;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) if (!__builtin_isfinite(T.a[i][j])) return false;
    if (!real_schur(T, U, n)) return false;
    for (int i = 0; i < n;) {
        if (i == n - 1 || T.a[i + 1][i] == 0.f) { re[i] = T.a[i][i]; im[i] = 0.f; ++i; continue; }
        const float a = T.a[i][i], b = T.a[i][i + 1], c = T.a[i + 1][i], d = T.a[i + 1][i + 1];
        const float p = 0.5f * (a - d), q = p * p + b * c;
        const float z = sqrtf(fabsf(q));
        re[i] = re[i + 1] = d + p; im[i] = z; im[i + 1] = -z;
        i += 2;
    }
    return true;
}

// A^-1 B by Gaussian elimination with partial pivoting (4 x 4)
CVO_HD void solve(M4 A, M4 B, M4& X) {
    const int n = 4;
    for (int c = 0; c < n; ++c) {
        int piv = c; for (int r = c + 1; r < n; ++r) if (fabsf(A.a[r][c]) > fabsf(A.a[piv][c])) piv = r;
        if (piv != c) for (int k = 0; k < n; ++k) {
            const float ta = A.a[c][k]; A.a[c][k] = A.a[piv][k]; A.a[piv][k] = ta;
            const float tb = B.a[c][k]; B.a[c][k] = B.a[piv][k]; B.a[piv][k] = tb;
        }
        for (int r = c + 1; r < n; ++r) {
            const float f = A.a[r][c] / A.a[c][c];
            for (int k = c; k < n; ++k) A.a[r][k] -= f * A.a[c][k];
            for (int k = 0; k < n; ++k) B.a[r][k] -= f * B.a[c][k];
        }
    }
    for (int c = n - 1; c >= 0; --c)
        for (int k = 0; k < n; ++k) {
            float s = B.a[c][k]; for (int j = c + 1; j < n; ++j) s -= A.a[c][j] * B.a[j][k];
            B.a[c][k] = s / A.a[c][c];
        }
    X = B;
}

CVO_HD float norm1_minus_identity(const M4& A) {
    float best = 0.f;
    for (int c = 0; c < 4; ++c) { float s = 0.f; for (int r = 0; r < 4; ++r) s += fabsf(A.a[r][c] - ((r == c) ? 1.f : 0.f)); best = fmax_std(best, s); }
    return best;
}

// principal square root by the Denman-Beavers iteration (product-free form)
CVO_HD void sqrt_db(M4& Y) {
    M4 Z, I, Yi, Zi;
    m4_identity(Z); m4_identity(I);
    for (int it = 0; it < 50; ++it) {
        solve(Y, I, Yi); solve(Z, I, Zi);
        float delta = 0.f;
        M4 Yn = Y, Zn = Z;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
            Yn.a[i][j] = 0.5f * (Y.a[i][j] + Zi.a[i][j]); Zn.a[i][j] = 0.5f * (Z.a[i][j] + Yi.a[i][j]);
            delta = fmax_std(delta, fabsf(Yn.a[i][j] - Y.a[i][j]));
        }
        Y = Yn; Z = Zn;
        if (delta <= 4.f * FLT_EPS) break;
    }
}

// log(A) of a 4 x 4 by inverse scaling and squaring on the real Schur form: out = U log(T) U^T
CVO_HD bool logm4(const M4& A, M4& out) {
    M4 T = A, U;
    if (!real_schur(T, U, 4)) return false;
    const float thr0 = (float)2.5111573934555054e-1, thr1 = (float)4.0535837411880493e-1, thr2 = (float)5.3149729967117310e-1;
    int roots = 0;
    float nrm = norm1_minus_identity(T);
    while (!(nrm < thr2)) {
        if (roots > 40 || !__builtin_isfinite(nrm)) return false;
        sqrt_db(T); ++roots;
        nrm = norm1_minus_identity(T);
    }
    const int deg = !(nrm <= thr0) ? (!(nrm <= thr1) ? 5 : 4) : 3;
    // Gauss-Legendre nodes and weights on [0, 1] of degree 3, 4, 5
    float node[5], weight[5];
    if (deg == 3) {
        node[0] = (float)0.1127016653792583114820734600217600; node[1] = (float)0.5; node[2] = (float)0.8872983346207416885179265399782400;
        weight[0] = (float)0.2777777777777777777777777777777778; weight[1] = (float)0.4444444444444444444444444444444444; weight[2] = (float)0.2777777777777777777777777777777778;
    } else if (deg == 4) {
        node[0] = (float)0.0694318442029737123880267555535953; node[1] = (float)0.3300094782075718675986671204483777;
        node[2] = (float)0.6699905217924281324013328795516223; node[3] = (float)0.9305681557970262876119732444464048;
        weight[0] = (float)0.1739274225687269286865319746109997; weight[1] = (float)0.3260725774312730713134680253890003;
        weight[2] = (float)0.3260725774312730713134680253890003; weight[3] = (float)0.1739274225687269286865319746109997;
    } else {
        node[0] = (float)0.0469100770306680036011865608503035; node[1] = (float)0.2307653449471584544818427896498956; node[2] = (float)0.5;
        node[3] = (float)0.7692346550528415455181572103501044; node[4] = (float)0.9530899229693319963988134391496965;
        weight[0] = (float)0.1184634425280945437571320203599587; weight[1] = (float)0.2393143352496832340206457574178191;
        weight[2] = (float)0.2844444444444444444444444444444444; weight[3] = (float)0.2393143352496832340206457574178191;
        weight[4] = (float)0.1184634425280945437571320203599587;
    }
    M4 X = T; for (int i = 0; i < 4; ++i) X.a[i][i] -= 1.f;
    M4 L; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) L.a[i][j] = 0.f;
    for (int k = 0; k < deg; ++k) {
        M4 M, Y; m4_identity(M);
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) M.a[i][j] += node[k] * X.a[i][j];
        solve(M, X, Y);
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) L.a[i][j] += weight[k] * Y.a[i][j];
    }
    const float scale = ldexpf(1.f, roots);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) L.a[i][j] *= scale;
    M4 Ut, UL; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Ut.a[i][j] = U.a[j][i];
    m4_mul(U, L, 4, UL);
    m4_mul(UL, Ut, 4, out);
    return true;
}

}  // namespace e337

// step of compute_step_size (cvo.cpp:317-333) with poly_solver's f32 eigenvalues (cvo.cpp:76-92): CVO_ARITH_F32_ROOTS
CVO_HD float cubic_step_f32eig(float c3, float c2, float c1, float c0, float min_step) {
    e337::M4 M;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) M.a[i][j] = 0.f;
    M.a[1][0] = 1.f; M.a[2][1] = 1.f;                                   // bottomLeftCorner = Identity, cvo.cpp:82-83
    M.a[0][0] = -(c2 / c3); M.a[0][1] = -(c1 / c3); M.a[0][2] = -(c0 / c3);   // M.row(0) = -(coef/coef(0)).segment(1, order), cvo.cpp:86
    float re[3], im[3];
    const float FMAX = 3.402823466e+38f;
    float best = FMAX;
    if (e337::eigenvalues(M, 3, re, im)) {
        for (int k = 0; k < 3; ++k) if (re[k] > 0 && re[k] < best && im[k] == 0) best = re[k];   // cvo.cpp:325-327
    }
    float step = (best == FMAX) ? min_step : best;                       // cvo.cpp:330
    step = step > 0.8 ? (float)0.8 : step;                               // cvo.cpp:333
    return step;
}

// dist_se3 (cvo.cpp:94-104) as Matrix4f::log().norm() in f32: CVO_ARITH_F32_LOGM.  NaN if the logarithm fails.
CVO_HD float dist_se3_f32logm(const float* dR, const float* dT) {
    e337::M4 M, Lg;
    e337::m4_identity(M);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) M.a[r][c] = dR[r * 3 + c]; M.a[r][3] = dT[r]; }
    if (!e337::logm4(M, Lg)) return __builtin_nanf("");
    float s = 0.f;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) s += Lg.a[r][c] * Lg.a[r][c];
    return sqrtf(s);
}

}  // namespace cvohip
