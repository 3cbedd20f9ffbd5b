// salsa_math.h -- per-thread arithmetic of the MI355X SALSA kernels (host+device inline templates).
//
// Everything here is register-level math with no memory traffic: the radix-8/4 butterflies of the LDS-staged FFT, the
// packed-real-FFT unpack, the 4x4 Hermitian covariance / eigen-gate / principal-eigenvector solver and the FOA / MIC
// normalisations.  The kernels (salsa_kernels.hip, fused_kernel.hip, multichannel.hip) own all addressing and
// staging.  The same header compiles with g++ (tests/hostemu) so this arithmetic is unit-tested on CPU against the oracle before it ever runs on a GPU; that
// host build is a test harness, never a fallback of the product.
//
// Reference semantics implemented (paths relative to the upstream repo):
//   dataset/salsa_feature_extraction.py:99-127  covariance, coherence gate s0 > s1*cond, FOA / MIC normalisation
//   dataset/salsa_feature_extraction.py:53-93   3-frame RMS + noise-floor tracker step
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SALSA_HD __host__ __device__ __forceinline__
#else
#define SALSA_HD inline
#endif

namespace salsa {

template <typename T> struct cplx { T re, im; };

template <typename T> SALSA_HD cplx<T> cmul(cplx<T> a, cplx<T> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename T> SALSA_HD cplx<T> cmulc(cplx<T> a, cplx<T> b) { return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; } // a*conj(b)
template <typename T> SALSA_HD cplx<T> cadd(cplx<T> a, cplx<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> SALSA_HD cplx<T> csub(cplx<T> a, cplx<T> b) { return {a.re - b.re, a.im - b.im}; }
template <typename T> SALSA_HD cplx<T> cconj(cplx<T> a) { return {a.re, -a.im}; }
template <typename T> SALSA_HD cplx<T> cmul_mi(cplx<T> a) { return {a.im, -a.re}; } // a * (-i)

// ---------------------------------------------------------------------------------------------------------------
// np.pad(mode='reflect') index (librosa.stft center=True): period 2N-2, no edge duplication.
SALSA_HD long reflect_index(long i, long N)
{
    if (i >= 0 && i < N) return i;
    if (N == 1) return 0;
    long p = 2 * (N - 1);
    i %= p;
    if (i < 0) i += p;
    return i < N ? i : p - i;
}

// ---------------------------------------------------------------------------------------------------------------
// In-register forward DFTs (decimation in frequency).  Outputs in natural order.
template <typename T> SALSA_HD void dft2(cplx<T> &a, cplx<T> &b)
{
    cplx<T> t = a;
    a = cadd(t, b);
    b = csub(t, b);
}

template <typename T> SALSA_HD void dft4(cplx<T> *x) // x[0..3] -> X[0..3]
{
    cplx<T> e0 = cadd(x[0], x[2]), o0 = csub(x[0], x[2]);
    cplx<T> e1 = cadd(x[1], x[3]), o1 = cmul_mi(csub(x[1], x[3]));
    x[0] = cadd(e0, e1);
    x[2] = csub(e0, e1);
    x[1] = cadd(o0, o1);
    x[3] = csub(o0, o1);
}

template <typename T> SALSA_HD void dft8(cplx<T> *x) // x[0..7] -> X[0..7]
{
    const T h = (T)0.70710678118654752440;
    cplx<T> s[4], d[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        s[j] = cadd(x[j], x[j + 4]);
        d[j] = csub(x[j], x[j + 4]);
    }
    // d[j] *= W8^j : W8^1 = (1-i)/sqrt2, W8^2 = -i, W8^3 = (-1-i)/sqrt2
    d[1] = {(d[1].re + d[1].im) * h, (d[1].im - d[1].re) * h};
    d[2] = cmul_mi(d[2]);
    d[3] = {(d[3].im - d[3].re) * h, -(d[3].re + d[3].im) * h};
    dft4(s);
    dft4(d);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        x[2 * m] = s[m];
        x[2 * m + 1] = d[m];
    }
}

template <int R, typename T> SALSA_HD void dftR(cplx<T> *x)
{
    if (R == 8) dft8(x);
    else if (R == 4) dft4(x);
    else dft2(x[0], x[1]);
}

// Two real channels packed as z = x0 + i*x1, Z = FFT(z).  a = Z[k], b = Z[(N-k) mod N]:
//   X0[k] = (a + conj(b))/2 ,  X1[k] = (a - conj(b))/(2i)
template <typename T> SALSA_HD void unpack_pair(cplx<T> a, cplx<T> b, cplx<T> &x0, cplx<T> &x1)
{
    x0 = {(a.re + b.re) * (T)0.5, (a.im - b.im) * (T)0.5};
    x1 = {(a.im + b.im) * (T)0.5, (b.re - a.re) * (T)0.5};
}

// Same with the /2 already applied to the transform's input (the kernels fold 0.5 into the window: exact).
template <typename T> SALSA_HD void unpack_pair_prescaled(cplx<T> a, cplx<T> b, cplx<T> &x0, cplx<T> &x1)
{
    x0 = {a.re + b.re, a.im - b.im};
    x1 = {a.im + b.im, b.re - a.re};
}

// ---------------------------------------------------------------------------------------------------------------
// 4x4 Hermitian matrix: 4 real diagonals + 6 complex upper off-diagonals in the order (01,02,03,12,13,23).
template <typename T> struct herm4 {
    T d[4];
    cplx<T> o[6];
};

// acc += x x^H  (x = 4 channels of one frame).  salsa_feature_extraction.py:99-100 (the /7 is a common scale that
// neither the gate s0 > s1*cond nor the eigenvector depends on; it is dropped).
template <typename T> SALSA_HD void herm4_rank1_add(herm4<T> &A, const cplx<T> *x)
{
#pragma unroll
    for (int i = 0; i < 4; i++) A.d[i] += x[i].re * x[i].re + x[i].im * x[i].im;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++, k++) {
            A.o[k].re += x[i].re * x[j].re + x[i].im * x[j].im;
            A.o[k].im += x[i].im * x[j].re - x[i].re * x[j].im;
        }
}

// C = A*A (Hermitian)
template <typename T> SALSA_HD herm4<T> herm4_square(const herm4<T> &A)
{
    herm4<T> C;
    const cplx<T> a01 = A.o[0], a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4], a23 = A.o[5];
    T n01 = a01.re * a01.re + a01.im * a01.im, n02 = a02.re * a02.re + a02.im * a02.im;
    T n03 = a03.re * a03.re + a03.im * a03.im, n12 = a12.re * a12.re + a12.im * a12.im;
    T n13 = a13.re * a13.re + a13.im * a13.im, n23 = a23.re * a23.re + a23.im * a23.im;
    C.d[0] = A.d[0] * A.d[0] + n01 + n02 + n03;
    C.d[1] = A.d[1] * A.d[1] + n01 + n12 + n13;
    C.d[2] = A.d[2] * A.d[2] + n02 + n12 + n23;
    C.d[3] = A.d[3] * A.d[3] + n03 + n13 + n23;
    cplx<T> t;
    T s;
    s = A.d[0] + A.d[1]; t = cadd(cmulc(a02, a12), cmulc(a03, a13));            // a02 conj(a12) + a03 conj(a13)
    C.o[0] = {a01.re * s + t.re, a01.im * s + t.im};
    s = A.d[0] + A.d[2]; t = cadd(cmul(a01, a12), cmulc(a03, a23));             // a01 a12 + a03 conj(a23)
    C.o[1] = {a02.re * s + t.re, a02.im * s + t.im};
    s = A.d[0] + A.d[3]; t = cadd(cmul(a01, a13), cmul(a02, a23));              // a01 a13 + a02 a23
    C.o[2] = {a03.re * s + t.re, a03.im * s + t.im};
    s = A.d[1] + A.d[2]; t = cadd(cmul(cconj(a01), a02), cmulc(a13, a23));      // conj(a01) a02 + a13 conj(a23)
    C.o[3] = {a12.re * s + t.re, a12.im * s + t.im};
    s = A.d[1] + A.d[3]; t = cadd(cmul(cconj(a01), a03), cmul(a12, a23));       // conj(a01) a03 + a12 a23
    C.o[4] = {a13.re * s + t.re, a13.im * s + t.im};
    s = A.d[2] + A.d[3]; t = cadd(cmul(cconj(a02), a03), cmul(cconj(a12), a13)); // conj(a02) a03 + conj(a12) a13
    C.o[5] = {a23.re * s + t.re, a23.im * s + t.im};
    return C;
}

template <typename T> SALSA_HD T herm4_frob2(const herm4<T> &A) // ||A||_F^2 = tr(A^2)
{
    T s = A.d[0] * A.d[0] + A.d[1] * A.d[1] + A.d[2] * A.d[2] + A.d[3] * A.d[3];
    T o = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) o += A.o[k].re * A.o[k].re + A.o[k].im * A.o[k].im;
    return s + 2 * o;
}

template <typename T> SALSA_HD T herm4_trace_prod(const herm4<T> &A, const herm4<T> &B) // tr(A B)
{
    T s = A.d[0] * B.d[0] + A.d[1] * B.d[1] + A.d[2] * B.d[2] + A.d[3] * B.d[3];
    T o = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) o += A.o[k].re * B.o[k].re + A.o[k].im * B.o[k].im;
    return s + 2 * o;
}

// element (i,j) of a Hermitian matrix from its packed upper triangle
template <typename T> SALSA_HD cplx<T> herm4_at(const herm4<T> &A, int i, int j)
{
    if (i == j) return {A.d[i], (T)0};
    const int idx[4][4] = {{-1, 0, 1, 2}, {0, -1, 3, 4}, {1, 3, -1, 5}, {2, 4, 5, -1}};
    cplx<T> v = A.o[idx[i][j]];
    return i < j ? v : cconj(v);
}

template <typename T> SALSA_HD cplx<T> det3(cplx<T> a, cplx<T> b, cplx<T> c, cplx<T> d, cplx<T> e, cplx<T> f, cplx<T> g,
                                            cplx<T> h, cplx<T> i)
{
    // | a b c ; d e f ; g h i |
    cplx<T> m0 = csub(cmul(e, i), cmul(f, h));
    cplx<T> m1 = csub(cmul(d, i), cmul(f, g));
    cplx<T> m2 = csub(cmul(d, h), cmul(e, g));
    return cadd(csub(cmul(a, m0), cmul(b, m1)), cmul(c, m2));
}

// ---------------------------------------------------------------------------------------------------------------
// Cheap reciprocal / reciprocal-sqrt (device: v_rcp_f64 / v_rsq_f64, ~24 good bits).  Used only where the
// consumer is self-correcting (Newton root iteration) or where the seed is refined explicitly.
SALSA_HD double approx_rcp(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcp(x);
#else
    return 1.0 / x;
#endif
}
SALSA_HD double approx_rsqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsq(x);
#else
    return 1.0 / sqrt(x);
#endif
}
// 1/sqrt(x) to ~1e-15 relative: hardware seed + two Newton steps.  x = 0 -> NaN after refinement (inf * NaN), the
// same NaN the reference's 0/0 produces at salsa_feature_extraction.py:119.
SALSA_HD double refined_rsqrt(double x)
{
    double y = approx_rsqrt(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    return y;
}
// 2^(-floor(log2 x)) for normal positive x: scaling by it is exact and puts x in [1, 2).
SALSA_HD double pow2_unscale(double x)
{
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    const uint64_t e = (bits >> 52) & 0x7ff;
    return __builtin_bit_cast(double, (uint64_t)(2046 - e) << 52);
}

// The twelve 2x2 minors (rows {0,1}: s0..s5, rows {2,3}: c0..c5) of a Hermitian 4x4 in packed form, from which both
// the characteristic polynomial and the adjugate follow by Laplace expansion.
template <typename T> struct minors4 {
    T s0, c5;                          // real for a Hermitian matrix
    cplx<T> s1, s2, s3, s4, s5, c0, c1, c2, c3, c4;
};

template <typename T> SALSA_HD cplx<T> rmul(T r, cplx<T> a) { return {r * a.re, r * a.im}; }

template <typename T> SALSA_HD minors4<T> herm4_minors(const herm4<T> &A)
{
    const T a00 = A.d[0], a11 = A.d[1], a22 = A.d[2], a33 = A.d[3];
    const cplx<T> a01 = A.o[0], a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4], a23 = A.o[5];
    minors4<T> m;
    m.s0 = a00 * a11 - (a01.re * a01.re + a01.im * a01.im);
    m.s1 = csub(rmul(a00, a12), cmul(cconj(a01), a02));          // a00 a12 - a10 a02
    m.s2 = csub(rmul(a00, a13), cmul(cconj(a01), a03));          // a00 a13 - a10 a03
    m.s3 = csub(cmul(a01, a12), rmul(a11, a02));                 // a01 a12 - a11 a02
    m.s4 = csub(cmul(a01, a13), rmul(a11, a03));                 // a01 a13 - a11 a03
    m.s5 = csub(cmul(a02, a13), cmul(a12, a03));                 // a02 a13 - a12 a03
    m.c5 = a22 * a33 - (a23.re * a23.re + a23.im * a23.im);
    m.c4 = csub(rmul(a33, cconj(a12)), cmul(cconj(a13), a23));   // a21 a33 - a31 a23
    m.c3 = csub(cmul(cconj(a12), cconj(a23)), rmul(a22, cconj(a13))); // a21 a32 - a31 a22
    m.c2 = csub(rmul(a33, cconj(a02)), cmul(cconj(a03), a23));   // a20 a33 - a30 a23
    m.c1 = csub(cmul(cconj(a02), cconj(a23)), rmul(a22, cconj(a03))); // a20 a32 - a30 a22
    m.c0 = csub(cmul(cconj(a02), cconj(a13)), cmul(cconj(a03), cconj(a12))); // a20 a31 - a30 a21
    return m;
}

template <typename T> SALSA_HD T re_mul(cplx<T> a, cplx<T> b) { return a.re * b.re - a.im * b.im; } // Re(a b)

// diagonal of adj(A) (real) from the minors
template <typename T> SALSA_HD void herm4_adj_diag(const herm4<T> &A, const minors4<T> &m, T *dg)
{
    const cplx<T> a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4];
    dg[0] = A.d[1] * m.c5 - re_mul(a12, m.c4) + re_mul(a13, m.c3);                       //  a11 c5 - a12 c4 + a13 c3
    dg[1] = A.d[0] * m.c5 - re_mul(a02, m.c2) + re_mul(a03, m.c1);                       //  a00 c5 - a02 c2 + a03 c1
    dg[2] = re_mul(cconj(a03), m.s4) - re_mul(cconj(a13), m.s2) + A.d[3] * m.s0;         //  a30 s4 - a31 s2 + a33 s0
    dg[3] = re_mul(cconj(a02), m.s3) - re_mul(cconj(a12), m.s1) + A.d[2] * m.s0;         //  a20 s3 - a21 s1 + a22 s0
}

// The coherence test decided ON THE MATRIX (round 6): eigenvalues of a Hermitian 4x4 by cyclic complex Jacobi rotations (what the CPU
// oracle uses for np.linalg.svd, accurate to ~1e-16 ||A|| whatever the eigenvalue multiplicities) -> s0 > s1 * cond
// (salsa_feature_extraction.py:106).  The quartic's Taylor coefficients cannot decide the test when the threshold mu1 / cond sits on a
// MULTIPLE root: with mu2 ~ mu3 (~ mu4) the value q(c) is a product of two (three) small factors, so float64 resolves mu1 / mu2
// against cond only to ~sqrt(eps) (eps^(1/3)) -- found by tests/test_gpu_pk_stress.py's `degenerate_tail` family, where the float64
// gate flipped against the oracle at margins of 7e-6.  Used when |q(c)| < SALSA_GATE_DOUBT, i.e. when c is numerically ON a root:
// never on natural signals (|mu1 / cond - mu2| < ~3e-11 for a simple mu2).  On the device herm4_gate_eigvec only FLAGS such a bin
// (eig_result::doubt; inlining ~600 instructions of rotations took the production kernel from 128 to 150 VGPRs + scratch): the
// kernels record it in a bit mask and gate_doubt_kernel (salsa_kernels.hip) decides it here after the launch.  On the host
// (tests/hostemu) the call is made in place.
#ifndef SALSA_GATE_DOUBT
#define SALSA_GATE_DOUBT 1e-12   // on the trace-1..2 scale; q(c) is evaluated to ~1e-14 there (64 operations on terms <= 1.5)
#endif
SALSA_HD bool herm4_rank1_by_jacobi(const herm4<double> &A, double cond)
{
    double ar[4][4], ai[4][4];
    {
        int k = 0;
        for (int i = 0; i < 4; i++) {
            ar[i][i] = A.d[i];
            ai[i][i] = 0.0;
            for (int j = i + 1; j < 4; j++, k++) {
                ar[i][j] = A.o[k].re; ai[i][j] = A.o[k].im;
                ar[j][i] = A.o[k].re; ai[j][i] = -A.o[k].im;
            }
        }
    }
    const double tr = ar[0][0] + ar[1][1] + ar[2][2] + ar[3][3];
    for (int sweep = 0; sweep < 12; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 4; p++)
            for (int q = p + 1; q < 4; q++) off += ar[p][q] * ar[p][q] + ai[p][q] * ai[p][q];
        if (off <= 1e-34 * tr * tr) break;
        for (int p = 0; p < 4; p++)
            for (int q = p + 1; q < 4; q++) {
                const double xr = ar[p][q], xi = ai[p][q];
                const double r2 = xr * xr + xi * xi;
                if (r2 == 0.0) continue;
                const double r = sqrt(r2);
                // a_pq = r e^{i phi}; U = D G with D_qq = e^{-i phi} (makes the pivot real) and G the real rotation that zeroes it
                const double er = xr / r, ei = xi / r;
                const double tau = (ar[q][q] - ar[p][p]) / (2.0 * r);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
                const double uqp_r = -sn * er, uqp_i = sn * ei, uqq_r = c * er, uqq_i = -c * ei;
                for (int i = 0; i < 4; i++) { // A <- A U (columns p, q)
                    const double pr = ar[i][p], pi = ai[i][p], qr = ar[i][q], qi = ai[i][q];
                    ar[i][p] = pr * c + (qr * uqp_r - qi * uqp_i);
                    ai[i][p] = pi * c + (qr * uqp_i + qi * uqp_r);
                    ar[i][q] = pr * sn + (qr * uqq_r - qi * uqq_i);
                    ai[i][q] = pi * sn + (qr * uqq_i + qi * uqq_r);
                }
                for (int j = 0; j < 4; j++) { // A <- U^H A (rows p, q)
                    const double pr = ar[p][j], pi = ai[p][j], qr = ar[q][j], qi = ai[q][j];
                    ar[p][j] = c * pr + (uqp_r * qr + uqp_i * qi);
                    ai[p][j] = c * pi + (uqp_r * qi - uqp_i * qr);
                    ar[q][j] = sn * pr + (uqq_r * qr + uqq_i * qi);
                    ai[q][j] = sn * pi + (uqq_r * qi - uqq_i * qr);
                }
                ar[p][q] = ai[p][q] = ar[q][p] = ai[q][p] = 0.0;
                ai[p][p] = ai[q][q] = 0.0;
            }
    }
    int i1 = 0;
    double l1 = ar[0][0];
    for (int i = 1; i < 4; i++)
        if (ar[i][i] > l1) { l1 = ar[i][i]; i1 = i; }
    double l2 = -1e300;
    for (int i = 0; i < 4; i++)
        if (i != i1 && ar[i][i] > l2) l2 = ar[i][i];
    return l1 > l2 * cond;
}
// Result of the per-TF-bin solve.
template <typename T> struct eig_result {
    bool rank1;      // coherence test s0 > s1*cond (salsa_feature_extraction.py:106)
    T margin;        // diagnostic: q(mu1/cond) (negative = exactly one root above the threshold)
    cplx<T> u[4];    // principal eigenvector (arbitrary scale and phase); valid when computed
    bool col0;       // u is column 0 of adj(A - mu1 I): u[0] is REAL (its imaginary part is exactly 0)
    bool fallback;   // PATH 1 only: the bin passed the gate but its column-0 pivot is too small -- solve it again with PATH 2
    bool doubt;      // device only: |q(mu1/cond)| < SALSA_GATE_DOUBT, rank1 is provisional -- herm4_rank1_by_jacobi decides (gate_doubt_kernel)
};

// Gate + principal eigenvector of a Hermitian PSD 4x4 R (any positive scale).
//
// Eigenvalues: R is scaled by an exact power of two so its trace lies in [1,2) (A).  The characteristic quartic
//   q(x) = x^4 - e1 x^3 + e2 x^2 - e3 x + e4,  e1 = tr A, e2 = sum of principal 2x2 minors, e3 = tr adj(A), e4 = det A
// comes from the 2x2 minors by Laplace expansion.  mu1 = largest root by Newton's iteration started just above
// sqrt(tr A^2) >= mu1, which descends monotonically onto mu1 for a real-rooted polynomial (the division inside the
// iteration may be approximate: the iteration is self-correcting).  The gate mu1 > cond*mu2 is decided WITHOUT
// solving for mu2: by Budan-Fourier (exact for real-rooted polynomials) the number of roots above c = mu1/cond equals
// the sign variations of the Taylor coefficients (q, q1, q2/2, q3/6, 1) of q at c; the bin is rank-1 iff that count
// is exactly one.
// Eigenvector: a column of adj(A - mu1 I) = prod_{i>=2}(mu_i - mu1) u u^H (again from 2x2 minors), taking the column
// with the largest diagonal cofactor.  Exact for any spectral gap (also with tracking off, where nothing gates it).
//
// Gated fast path (round 3).  A bin that passed the gate has a simple mu1 with gap mu1 - mu2 > (1 - 1/cond) mu1, so
// adj(A - mu1 I) = prod_{i>=2}(mu_i - mu1) u u^H is a well-scaled rank-1 matrix and ANY column whose pivot u_j is not tiny
// is an accurate eigenvector.  Column 0 needs one real and three complex cofactors (6 of the 12 shifted minors) instead of
// four diagonal cofactors, an arg-max and six complex cofactors folded through selects; its pivot adj_00 = prod * |u_0|^2 is
// REAL, which the FOA / MIC normalisations use (Re(u_i conj(u_0)) = adj_00 Re(u_i)).  Taken when |adj_00| >= SALSA_COL0_MIN
// on the trace-1..2 scale (relative error of the column <~ 1e-15 / |adj_00|); smaller pivots (u_0 ~ 0: the FOA feature is
// ill-conditioned there anyway) and the ungated mode (no gap guarantee) take the general arg-max path below, unchanged.
#ifndef SALSA_COL0_MIN
#define SALSA_COL0_MIN 1e-6
#endif
#ifndef SALSA_COL0
#define SALSA_COL0 1
#endif
// PATH selects what is COMPILED: 0 = fast path with the general path behind it (one call does everything; host harness),
// 1 = fast path only (the kernel's hot loop: a gated bin whose pivot is too small comes back with `fallback` set and no
// vector, to be re-solved by a PATH-2 call in the kernel's cold loop -- the hot loop then carries neither the general path's
// instructions nor its registers), 2 = general path only (the cold loop, and the ungated mode).
template <int PATH = 0, typename T>
SALSA_HD eig_result<T> herm4_gate_eigvec(const herm4<T> &R, T cond, T inv_cond, bool need_vector_always, bool want_imag = true)
{
    eig_result<T> res;
    res.rank1 = false;
    res.col0 = false;
    res.fallback = false;
    res.doubt = false;
    res.margin = 0;
    res.u[0] = {(T)1, (T)0};
    res.u[1] = res.u[2] = res.u[3] = {(T)0, (T)0};
    const T tr = R.d[0] + R.d[1] + R.d[2] + R.d[3];
    if (!(tr > (T)0)) return res; // zero matrix: s0 > s1*cond is 0 > 0 = False; LAPACK's U for it is the identity
    const T sc = (T)pow2_unscale((double)tr);
    herm4<T> A;
#pragma unroll
    for (int i = 0; i < 4; i++) A.d[i] = R.d[i] * sc;
#pragma unroll
    for (int k = 0; k < 6; k++) A.o[k] = {R.o[k].re * sc, R.o[k].im * sc};
    T nrm = 0; // sum |a_ij|^2, i<j
#pragma unroll
    for (int k = 0; k < 6; k++) nrm += A.o[k].re * A.o[k].re + A.o[k].im * A.o[k].im;
    const T e1 = A.d[0] + A.d[1] + A.d[2] + A.d[3];
    const T e2 = A.d[0] * A.d[1] + A.d[0] * A.d[2] + A.d[0] * A.d[3] + A.d[1] * A.d[2] + A.d[1] * A.d[3] + A.d[2] * A.d[3] - nrm;
    const T p2 = e1 * e1 - (T)2 * e2;             // tr(A^2) = sum mu_i^2 >= mu1^2
    if (!need_vector_always && cond > (T)1) {
        // Cheap certain-fail test before any minor is formed.  For a PSD spectrum with mu1 > cond*mu2 (>= cond*mu3,4)
        // and sum mu = e1, sum mu^2 is smallest at mu = e1*(cond,1,1,1)/(cond+3), i.e. tr(A^2) >= (cond^2+3)/(cond+3)^2
        // * e1^2.  Anything below that bound cannot pass the coherence test (flat, noise-like covariances).
        const T bound = (cond * cond + (T)3) / ((cond + (T)3) * (cond + (T)3));
        if (p2 < bound * e1 * e1 * (T)(1.0 - 1e-9)) return res;
    }
    const minors4<T> m = herm4_minors(A);
    T dg[4];
    herm4_adj_diag(A, m, dg);
    const T e3 = dg[0] + dg[1] + dg[2] + dg[3];
    // det = s0 c5 - s1 c4 + s2 c3 + s3 c2 - s4 c1 + s5 c0 (real for Hermitian A)
    const T e4 = m.s0 * m.c5 - re_mul(m.s1, m.c4) + re_mul(m.s2, m.c3) + re_mul(m.s3, m.c2) - re_mul(m.s4, m.c1) + re_mul(m.s5, m.c0);
    const T a3 = -e1, a2 = e2, a1 = -e3, a0 = e4; // q(x) = x^4 + a3 x^3 + a2 x^2 + a1 x + a0
    T x = p2 * (T)approx_rsqrt((double)p2) * (T)(1.0 + 1.0 / 1048576.0); // just above sqrt(p2)
    if (!(x < e1)) x = e1;
    for (int it = 0; it < 64; it++) {
        const T q = (((x + a3) * x + a2) * x + a1) * x + a0;
        const T dq = (((T)4 * x + (T)3 * a3) * x + (T)2 * a2) * x + a1;
        if (!(dq > (T)0)) break;
        const T step = q * (T)approx_rcp((double)dq);
        if (!(step > (T)0)) break; // at (or rounded past) the root
        const T xn = x - step;
        if (!(xn < x)) break;
        x = xn;
        if (step <= (T)8 * (sizeof(T) == 8 ? (T)2.2e-16 : (T)1.2e-7) * x) break;
    }
    const T mu1 = x;
    if (cond <= (T)1) {
        res.rank1 = mu1 > (T)0; // mu2*cond < mu1 whenever mu1 > 0 (cond == 1: strict s0 > s1, a measure-zero tie)
    } else {
        const T c = mu1 * inv_cond; // inv_cond = 1/cond from the host: a float64 divide is ~25 instructions per bin
        const T t0 = (((c + a3) * c + a2) * c + a1) * c + a0;
        const T t1 = (((T)4 * c + (T)3 * a3) * c + (T)2 * a2) * c + a1;
        const T t2 = ((T)6 * c + (T)3 * a3) * c + a2;
        const T t3 = (T)4 * c + a3;
        int var = 0;
        T prev = (T)1; // fourth Taylor coefficient of a monic quartic
        if (t3 != (T)0) { var += ((t3 < 0) != (prev < 0)); prev = t3; }
        if (t2 != (T)0) { var += ((t2 < 0) != (prev < 0)); prev = t2; }
        if (t1 != (T)0) { var += ((t1 < 0) != (prev < 0)); prev = t1; }
        if (t0 != (T)0) { var += ((t0 < 0) != (prev < 0)); prev = t0; }
        res.rank1 = (var == 1);
        res.margin = t0;
        if (sizeof(T) == 8 && fabs(t0) < (T)SALSA_GATE_DOUBT) { // c numerically ON a root of q: the quartic cannot tell
#if defined(__HIP_DEVICE_COMPILE__)
            res.doubt = true;
#else
            herm4<double> Ad;
            for (int i = 0; i < 4; i++) Ad.d[i] = (double)A.d[i];
            for (int k = 0; k < 6; k++) Ad.o[k] = {(double)A.o[k].re, (double)A.o[k].im};
            res.rank1 = herm4_rank1_by_jacobi(Ad, (double)cond);
#endif
        }
    }
    if (!res.rank1 && !need_vector_always) return res;
    // B = A - mu1 I ; adj(B) column with the largest |diagonal cofactor|.  Only the diagonal changes, so B's 2x2 minors
    // are A's plus terms linear (s0, c5: quadratic) in mu1; s5 and c0 contain no diagonal entry at all.
    herm4<T> B = A;
#pragma unroll
    for (int i = 0; i < 4; i++) B.d[i] -= mu1;
    if (SALSA_COL0 && PATH != 2 && !need_vector_always) {
        const cplx<T> a01 = A.o[0], a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4], a23 = A.o[5];
        const T c5 = B.d[2] * B.d[3] - (a23.re * a23.re + a23.im * a23.im);
        const cplx<T> c4 = {m.c4.re - mu1 * a12.re, m.c4.im + mu1 * a12.im}; // conj(a12) (a33-mu) - a31 a23
        const cplx<T> c3 = {m.c3.re + mu1 * a13.re, m.c3.im - mu1 * a13.im}; // a21 a32 - conj(a13) (a22-mu)
        const T p00 = B.d[1] * c5 - re_mul(a12, c4) + re_mul(a13, c3);       // adj_00 = b11 c5 - b12 c4 + b13 c3
        if (fabs(p00) >= (T)SALSA_COL0_MIN) {
            const cplx<T> s3 = {m.s3.re + mu1 * a02.re, m.s3.im + mu1 * a02.im}; // a01 a12 - (a11-mu) a02
            const cplx<T> s4 = {m.s4.re + mu1 * a03.re, m.s4.im + mu1 * a03.im}; // a01 a13 - (a11-mu) a03
            const cplx<T> s5 = m.s5;
            // adj_0b (b = 1..3), as in the general path; column 0 is u_b = adj_b0 = conj(adj_0b)
            //   adj_01 = -b01 c5 + b02 c4 - b03 c3 ; adj_02 = conj(b13) s5 - conj(b23) s4 + b33 s3 ; adj_03 = b22 s4 - conj(b12) s5 - b23 s3
            res.u[0] = {p00, (T)0};
            res.u[1].re = re_mul(a02, c4) - c5 * a01.re - re_mul(a03, c3);
            res.u[2].re = re_mul(cconj(a13), s5) - re_mul(cconj(a23), s4) + B.d[3] * s3.re;
            res.u[3].re = B.d[2] * s4.re - re_mul(cconj(a12), s5) - re_mul(a23, s3);
            if (want_imag) { // -Im(adj_0b)
                res.u[1].im = -((a02.re * c4.im + a02.im * c4.re) - c5 * a01.im - (a03.re * c3.im + a03.im * c3.re));
                res.u[2].im = -((a13.re * s5.im - a13.im * s5.re) - (a23.re * s4.im - a23.im * s4.re) + B.d[3] * s3.im);
                res.u[3].im = -(B.d[2] * s4.im - (a12.re * s5.im - a12.im * s5.re) - (a23.re * s3.im + a23.im * s3.re));
            } else {
                res.u[1].im = res.u[2].im = res.u[3].im = (T)0;
            }
            res.col0 = true;
            return res;
        }
    }
    if (PATH == 1) { // hot loop: leave the rare small-pivot bin (and nothing else) to the cold loop
        res.fallback = true;
        return res;
    }
    minors4<T> n = m;
    {
        const cplx<T> a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4];
        n.s0 = B.d[0] * B.d[1] - (A.o[0].re * A.o[0].re + A.o[0].im * A.o[0].im);
        n.c5 = B.d[2] * B.d[3] - (A.o[5].re * A.o[5].re + A.o[5].im * A.o[5].im);
        n.s1 = {m.s1.re - mu1 * a12.re, m.s1.im - mu1 * a12.im}; // (a00-mu) a12 - a10 a02
        n.s2 = {m.s2.re - mu1 * a13.re, m.s2.im - mu1 * a13.im}; // (a00-mu) a13 - a10 a03
        n.s3 = {m.s3.re + mu1 * a02.re, m.s3.im + mu1 * a02.im}; // a01 a12 - (a11-mu) a02
        n.s4 = {m.s4.re + mu1 * a03.re, m.s4.im + mu1 * a03.im}; // a01 a13 - (a11-mu) a03
        n.c4 = {m.c4.re - mu1 * a12.re, m.c4.im + mu1 * a12.im}; // conj(a12) (a33-mu) - a31 a23
        n.c3 = {m.c3.re + mu1 * a13.re, m.c3.im - mu1 * a13.im}; // a21 a32 - conj(a13) (a22-mu)
        n.c2 = {m.c2.re - mu1 * a02.re, m.c2.im + mu1 * a02.im}; // conj(a02) (a33-mu) - a30 a23
        n.c1 = {m.c1.re + mu1 * a03.re, m.c1.im - mu1 * a03.im}; // a20 a32 - conj(a03) (a22-mu)
    }
    T bd[4];
    herm4_adj_diag(B, n, bd);
    const cplx<T> b01 = B.o[0], b02 = B.o[1], b03 = B.o[2], b12 = B.o[3], b13 = B.o[4], b23 = B.o[5];
    const T m0 = fabs(bd[0]), m1 = fabs(bd[1]), m2 = fabs(bd[2]), m3 = fabs(bd[3]);
    int j = 0;
    T best = m0;
    if (m1 > best) { best = m1; j = 1; }
    if (m2 > best) { best = m2; j = 2; }
    if (m3 > best) { best = m3; j = 3; }
    // column j of adj(B): u_i = adj_{ij}; adj is Hermitian, so entry (a,b), a<b, serves column b directly and column a
    // conjugated.  Each entry is folded into u as soon as it is formed (keeps the live register set small).
    res.u[0] = {j == 0 ? bd[0] : (T)0, (T)0};
    res.u[1] = {j == 1 ? bd[1] : (T)0, (T)0};
    res.u[2] = {j == 2 ? bd[2] : (T)0, (T)0};
    res.u[3] = {j == 3 ? bd[3] : (T)0, (T)0};
    auto put = [&](const int a, const int b, const cplx<T> v) {
        if (j == b) res.u[a] = v;
        if (j == a) res.u[b] = cconj(v);
    };
    put(0, 1, csub(csub(cmul(b02, n.c4), rmul(n.c5, b01)), cmul(b03, n.c3)));                    // -a01 c5 + a02 c4 - a03 c3
    put(0, 2, cadd(csub(cmul(cconj(b13), n.s5), cmul(cconj(b23), n.s4)), rmul(B.d[3], n.s3)));   //  a31 s5 - a32 s4 + a33 s3
    put(0, 3, csub(csub(rmul(B.d[2], n.s4), cmul(cconj(b12), n.s5)), cmul(b23, n.s3)));          // -a21 s5 + a22 s4 - a23 s3
    put(1, 2, csub(csub(cmul(cconj(b23), n.s2), cmul(cconj(b03), n.s5)), rmul(B.d[3], n.s1)));   // -a30 s5 + a32 s2 - a33 s1
    put(1, 3, cadd(csub(cmul(cconj(b02), n.s5), rmul(B.d[2], n.s2)), cmul(b23, n.s1)));          //  a20 s5 - a22 s2 + a23 s1
    put(2, 3, csub(csub(cmul(cconj(b12), n.s2), cmul(cconj(b02), n.s4)), rmul(n.s0, b23)));      // -a20 s4 + a21 s2 - a23 s0
    if (!(best > (T)0)) { // A == mu1 I numerically (fully degenerate): any vector; match LAPACK's identity column
        res.u[0] = {(T)1, (T)0};
        res.u[1] = res.u[2] = res.u[3] = {(T)0, (T)0};
    }
    return res;
}

// FOA: real(u[1:]/u[0]) then L2-normalise (salsa_feature_extraction.py:118-119).  Re(u_i/u_0) = Re(u_i conj(u_0))
// / |u_0|^2 and the positive factor 1/|u_0|^2 cancels in the normalisation, so e = v/||v|| with v_i = Re(u_i
// conj(u_0)); u_0 = 0 gives 0/0 = NaN exactly where the reference (no guard) does.
template <typename T> SALSA_HD void normalise_foa(const cplx<T> *u, T *e, bool rescale = true)
{
    // scale u so |v| is O(1): adjugate columns can be tiny when the spectral gap is (tracking off, no gate).  With the
    // gate (mu1 > cond*mu2 on a trace-1..2 matrix) the chosen column is O(gap^3 |u_j|) >= 1e-2: no rescale needed.
    T s = 0;
    if (rescale) {
#pragma unroll
        for (int i = 0; i < 4; i++) { s = fmax(s, fabs(u[i].re)); s = fmax(s, fabs(u[i].im)); }
    }
    const T r = (rescale && s > (T)0) ? (T)pow2_unscale((double)s) : (T)1;
    const cplx<T> u0 = {u[0].re * r, u[0].im * r};
    T ss = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        e[i] = (u[i + 1].re * r) * u0.re + (u[i + 1].im * r) * u0.im;
        ss += e[i] * e[i];
    }
    const T inv = (T)refined_rsqrt((double)ss);
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = e[i] * inv;
}

// FOA from a column-0 eigenvector (eig_result::col0): u_0 = adj_00 is real, so Re(u_i conj(u_0)) = adj_00 Re(u_i) and the
// unit vector is sign(adj_00) Re(u[1:4]) / ||Re(u[1:4])||.  |adj_00| >= SALSA_COL0_MIN keeps everything O(1e-6..1): no rescale.
template <typename T> SALSA_HD void normalise_foa_col0(const cplx<T> *u, T *e)
{
    const T ss = u[1].re * u[1].re + u[2].re * u[2].re + u[3].re * u[3].re;
    T inv = (T)refined_rsqrt((double)ss);
    if (u[0].re < (T)0) inv = -inv;
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = u[i + 1].re * inv;
}

// MIC from a column-0 eigenvector: angle(u_i conj(u_0)) = angle(sign(adj_00) u_i).
template <typename T> SALSA_HD void normalise_mic_col0(const cplx<T> *u, T dk, T *e)
{
    const T sg = u[0].re < (T)0 ? (T)-1 : (T)1;
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = atan2(sg * u[i + 1].im, sg * u[i + 1].re) / dk;
}

// MIC: angle(u[1:]*conj(u[0])) / (delta*k) (salsa_feature_extraction.py:121-123); dk = delta*(ibin+lower_bin).
template <typename T> SALSA_HD void normalise_mic(const cplx<T> *u, T dk, T *e)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        cplx<T> w = cmulc(u[i + 1], u[0]);
        e[i] = atan2(w.im, w.re) / dk;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Packed-float32 pair solve (round 4).  A K3 work item is TWO neighbouring frames of one TF bin, i.e. two independent 4 x 4
// problems per lane.  pk2f holds one float32 of each (.x = frame t, .y = frame t + 1), so every arithmetic instruction below is
// a v_pk_{mul,add,fma}_f32 doing useful work in BOTH halves (gfx950 issues a packed float32 VALU instruction in the slot of one
// float64 or one scalar float32 instruction: this is the only float32 form that is faster than float64 there).  The covariance
// is still accumulated in float64 (products of float32 spectra are exact there), scaled by an exact power of two to a trace in
// [1, 2) and rounded ONCE to float32; the quartic, Newton, Budan-Fourier gate and column-0 adjugate then run as the float64
// code above does, on pairs.  What float32 cannot decide or deliver is handed back, per frame, in `unsure`:
//   * the gate, when a Taylor coefficient of q at mu1/cond that the sign-variation count depends on lies within
//     SALSA_PK_GATE_TOL of zero (coefficient errors are <= ~3e-6 on the trace-1..2 scale);
//   * the eigenvector, when the real pivot adj_00 = prod(mu_i - mu1) |u_0|^2 is below SALSA_PK_PIVOT_MIN (the column's relative
//     error grows as 1 / |adj_00|), and -- in the normalisations below -- when the feature itself is ill-conditioned.
// Those frames go to the kernel's float64 cold list; everything certified here agrees with the float64 gate bit for bit and
// with its features to well inside the test bar (tests/test_kernel_math_hostemu.py::test_packed_float32_pair_solve_*).
typedef float pk2f __attribute__((vector_size(8)));
SALSA_HD pk2f pk_splat(float a)
{
    pk2f r = {a, a};
    return r;
}
SALSA_HD float approx_rcpf(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
SALSA_HD float approx_rsqrtf(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(x);
#else
    return 1.0f / sqrtf(x);
#endif
}
#ifndef SALSA_PK_GATE_TOL
#define SALSA_PK_GATE_TOL 2e-5f
#endif
#ifndef SALSA_PK_NEWTON
#define SALSA_PK_NEWTON 5        // packed Newton iterations (the last one's step certifies convergence)
#endif
#ifndef SALSA_PK_PIVOT_MIN
#define SALSA_PK_PIVOT_MIN 1e-2f
#endif
#ifndef SALSA_PK_FOA_MIN
#define SALSA_PK_FOA_MIN 1e-2f   // FOA: ||Re(column 0)[1:4]||^2 below this -> float64
#endif
#ifndef SALSA_PK_MIC_MIN
#define SALSA_PK_MIC_MIN 1e-3f   // MIC: |column 0 entry|^2 below this -> float64 (the angle's error grows as 1 / |entry|)
#endif

struct pk_eig {
    int pass;          // bit j: frame j passed the coherence test (certified) and its column is in ur / ui
    int unsure;        // bit j: frame j must be solved again in float64
    pk2f p00;          // real pivot adj_00
    pk2f ur[3], ui[3]; // column 0 of adj(A - mu1 I), entries 1..3 (ui only when WANT_IMAG)
};

// Float32 covariance of ONE window in the (re, im) packing the spectra are loaded in: dsq[i] accumulates (re_i^2, im_i^2),
// o[k] the complex entry (i, j), i < j, as (re, im).  x_i conj(x_j) = (xi.re xj.re + xi.im xj.im, xi.im xj.re - xi.re xj.im) is
// two packed FMAs: splat(xi.re) * (xj.re, -xj.im) + splat(xi.im) * (xj.im, xj.re) -- the splat, the swap and the negation are
// operand modifiers (op_sel / neg_hi) of v_pk_fma_f32, so a frame costs 16 instructions where the float64 form costs 40.
struct cov4pk {
    pk2f dsq[4], o[6];
};
// acc + a conj(b) for (re, im) pairs.  Device: exactly two v_pk_fma_f32 -- left to the compiler, the negated and the swapped
// operand are materialised with v_xor / v_mov (measured: +6 instructions per frame).
SALSA_HD pk2f pk_cmac_conj(pk2f acc, pk2f a, pk2f b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    pk2f t, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(t) : "v"(a), "v"(b), "v"(acc));      // + a.re (b.re, -b.im)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));        // + a.im (b.im,  b.re)
    return r;
#else
    const pk2f bn = {b[0], -b[1]}, bs = {b[1], b[0]};
    return (acc + pk_splat(a[0]) * bn) + pk_splat(a[1]) * bs;
#endif
}
// out = in + v v^H (v[i] = (re, im) of channel i); out may alias in
SALSA_HD void cov4pk_rank1(cov4pk &out, const cov4pk &in, const pk2f *v)
{
#pragma unroll
    for (int i = 0; i < 4; i++) out.dsq[i] = in.dsq[i] + v[i] * v[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++, k++) out.o[k] = pk_cmac_conj(in.o[k], v[i], v[j]);
}
// 2^(-floor(log2 x)) for a normal positive float; `bad` set when x is zero / subnormal / huge / not finite
SALSA_HD float pow2_unscalef(float x, bool &bad)
{
    const uint32_t e = (__builtin_bit_cast(uint32_t, x) >> 23) & 0xffu;
    bad = bad || e < 2u || e > 252u;
    return __builtin_bit_cast(float, (uint32_t)(254u - e) << 23);
}
// The two windows' covariances -> the frame-pair packing of the solver (.x = window 0, .y = window 1), each scaled by an exact
// power of two to a trace in [1, 2).  Bit j of `odd` is set when window j's trace cannot be scaled in float32.
SALSA_HD herm4<pk2f> herm4_pk_from_windows(const cov4pk &R0, const cov4pk &R1, int &odd)
{
    herm4<pk2f> A;
#pragma unroll
    for (int i = 0; i < 4; i++) A.d[i] = pk2f{R0.dsq[i][0] + R0.dsq[i][1], R1.dsq[i][0] + R1.dsq[i][1]};
    const pk2f tr = (A.d[0] + A.d[1]) + (A.d[2] + A.d[3]);
    bool bad0 = false, bad1 = false;
    const pk2f sc = {pow2_unscalef(tr[0], bad0), pow2_unscalef(tr[1], bad1)};
    odd = (bad0 ? 1 : 0) | (bad1 ? 2 : 0);
#pragma unroll
    for (int i = 0; i < 4; i++) A.d[i] = A.d[i] * sc;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        A.o[k].re = pk2f{R0.o[k][0], R1.o[k][0]} * sc;
        A.o[k].im = pk2f{R0.o[k][1], R1.o[k][1]} * sc;
    }
    return A;
}

// Gate + column-0 eigenvector of two Hermitian PSD matrices whose traces were scaled into [1, 2).  `live`: bit j = frame j is
// wanted (the other lane may hold anything, NaN included: it is carried along and ignored).  cond > 1.
// `study` (host error study only, tools/pk_coeff_study.py; NULL in every kernel): receives the four Taylor coefficients t0..t3 of q at
// c = mu1 / cond, mu1, the last Newton step and c, as this float32 code computed them (the prefilter is bypassed so that every frame reports).
template <bool WANT_IMAG>
SALSA_HD pk_eig herm4_gate_eigvec_pk(const herm4<pk2f> &A, float cond, float inv_cond, int live, pk2f *study = nullptr)
{
    pk_eig res;
    res.pass = 0;
    res.unsure = 0;
    res.p00 = pk_splat(0.f);
#pragma unroll
    for (int i = 0; i < 3; i++) res.ur[i] = res.ui[i] = pk_splat(0.f);
    pk2f nrm = A.o[0].re * A.o[0].re + A.o[0].im * A.o[0].im;
#pragma unroll
    for (int k = 1; k < 6; k++) nrm = nrm + (A.o[k].re * A.o[k].re + A.o[k].im * A.o[k].im);
    const pk2f e1 = (A.d[0] + A.d[1]) + (A.d[2] + A.d[3]);
    const pk2f e2 = A.d[0] * A.d[1] + A.d[0] * A.d[2] + A.d[0] * A.d[3] + A.d[1] * A.d[2] + A.d[1] * A.d[3] + A.d[2] * A.d[3] - nrm;
    const pk2f p2 = e1 * e1 - 2.f * e2; // tr(A^2)
    // certain fail (see the float64 code): tr(A^2) >= (cond^2 + 3) / (cond + 3)^2 tr(A)^2 is necessary for passing; the float32
    // p2 carries ~5e-7 relative error, hence the 1e-5 slack.  A NaN lane fails here too.
    const float bound = (cond * cond + 3.f) / ((cond + 3.f) * (cond + 3.f)) * (1.f - 1e-5f);
    const pk2f need = bound * e1 * e1;
    int act = live;
#pragma unroll
    for (int j = 0; j < 2; j++)
        if (!(p2[j] >= need[j])) act &= ~(1 << j);
    if (!act && !study) return res;
    const minors4<pk2f> m = herm4_minors(A);
    pk2f dg[4];
    herm4_adj_diag(A, m, dg);
    const pk2f e3 = (dg[0] + dg[1]) + (dg[2] + dg[3]);
    const pk2f e4 = m.s0 * m.c5 - re_mul(m.s1, m.c4) + re_mul(m.s2, m.c3) + re_mul(m.s3, m.c2) - re_mul(m.s4, m.c1) + re_mul(m.s5, m.c0);
    const pk2f a3 = -e1, a2 = e2, a1 = -e3, a0 = e4;
    // Newton from just above sqrt(tr A^2) >= mu1, a FIXED number of packed iterations with no per-lane control: from above the
    // iterates descend monotonically onto mu1 (every one is an upper bound of it); a gated bin (mu2 < mu1 / cond) starts within
    // 6 % of mu1 and is at float32 accuracy after three steps.  The last evaluation's step is the convergence certificate.
    pk2f x;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        float x0 = p2[j] * approx_rsqrtf(p2[j]) * (1.f + 1.f / 65536.f); // (the seed and p2 are good to ~1e-6)
        if (!(x0 < e1[j])) x0 = e1[j];
        x[j] = x0;
    }
    const pk2f k3 = 3.f * a3, k2 = 2.f * a2;
    pk2f last = pk_splat(0.f);
#pragma unroll
    for (int it = 0; it < SALSA_PK_NEWTON; it++) {
        const pk2f q = (((x + a3) * x + a2) * x + a1) * x + a0;
        const pk2f dq = ((4.f * x + k3) * x + k2) * x + a1;
        const pk2f r = {approx_rcpf(dq[0]), approx_rcpf(dq[1])};
        last = q * r;
        x = x - last;
    }
    const pk2f mu1 = x;
    const pk2f c = mu1 * inv_cond;
    const pk2f t0 = (((c + a3) * c + a2) * c + a1) * c + a0;
    const pk2f t1 = ((4.f * c + k3) * c + k2) * c + a1;
    const pk2f t2 = (6.f * c + k3) * c + a2;
    const pk2f t3 = 4.f * c + a3;
    if (study) study[0] = t0, study[1] = t1, study[2] = t2, study[3] = t3, study[4] = mu1, study[5] = last, study[6] = c;
    int pass = 0, unsure = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (!((act >> j) & 1)) continue;
        const float tol = SALSA_PK_GATE_TOL;
        // q(c) > 0 for certain: an even number of roots above c, and mu1 is one of them -> at least two -> fails.  (Holds for an
        // unconverged x too: x >= mu1 puts c at or above the true threshold, which can only hide roots, not add them.)
        if (t0[j] >= tol) continue;
        const bool sure = fabsf(t0[j]) >= tol && fabsf(t1[j]) >= tol && fabsf(t2[j]) >= tol && fabsf(t3[j]) >= tol;
        int var = (t3[j] < 0.f);                  // against the leading 1
        var += (t2[j] < 0.f) != (t3[j] < 0.f);
        var += (t1[j] < 0.f) != (t2[j] < 0.f);
        var += (t0[j] < 0.f) != (t1[j] < 0.f);
        if (sure && var >= 2) continue;           // three roots above an upper bound of the threshold: fails, converged or not
        const bool conv = fabsf(last[j]) <= 4e-6f * mu1[j]; // (false for NaN)
        if (!sure || !conv || !(mu1[j] > 0.f)) {
            unsure |= 1 << j;
            continue;
        }
        if (var == 1) pass |= 1 << j;
    }
    res.unsure = unsure;
    if (!pass) return res;
    // column 0 of adj(A - mu1 I), as in the float64 fast path
    const pk2f b1 = A.d[1] - mu1, b2 = A.d[2] - mu1, b3 = A.d[3] - mu1;
    const cplx<pk2f> a01 = A.o[0], a02 = A.o[1], a03 = A.o[2], a12 = A.o[3], a13 = A.o[4], a23 = A.o[5];
    const pk2f c5 = b2 * b3 - (a23.re * a23.re + a23.im * a23.im);
    const cplx<pk2f> c4 = {m.c4.re - mu1 * a12.re, m.c4.im + mu1 * a12.im};
    const cplx<pk2f> c3 = {m.c3.re + mu1 * a13.re, m.c3.im - mu1 * a13.im};
    const pk2f p00 = b1 * c5 - re_mul(a12, c4) + re_mul(a13, c3);
    const cplx<pk2f> s3 = {m.s3.re + mu1 * a02.re, m.s3.im + mu1 * a02.im};
    const cplx<pk2f> s4 = {m.s4.re + mu1 * a03.re, m.s4.im + mu1 * a03.im};
    const cplx<pk2f> s5 = m.s5;
    res.p00 = p00;
    res.ur[0] = re_mul(a02, c4) - c5 * a01.re - re_mul(a03, c3);
    res.ur[1] = re_mul(cconj(a13), s5) - re_mul(cconj(a23), s4) + b3 * s3.re;
    res.ur[2] = b2 * s4.re - re_mul(cconj(a12), s5) - re_mul(a23, s3);
    if (WANT_IMAG) {
        res.ui[0] = -((a02.re * c4.im + a02.im * c4.re) - c5 * a01.im - (a03.re * c3.im + a03.im * c3.re));
        res.ui[1] = -((a13.re * s5.im - a13.im * s5.re) - (a23.re * s4.im - a23.im * s4.re) + b3 * s3.im);
        res.ui[2] = -(b2 * s4.im - (a12.re * s5.im - a12.im * s5.re) - (a23.re * s3.im + a23.im * s3.re));
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
        if (((pass >> j) & 1) && !(fabsf(p00[j]) >= SALSA_PK_PIVOT_MIN)) {
            pass &= ~(1 << j);
            res.unsure |= 1 << j;
        }
    res.pass = pass;
    return res;
}

// FOA feature of both frames from the packed column: e = sign(adj_00) Re(u[1:4]) / ||Re(u[1:4])|| (normalise_foa_col0).
// Frames whose ||.||^2 is below SALSA_PK_FOA_MIN are moved from `pass` to `unsure`.
SALSA_HD void normalise_foa_pk(pk_eig &r, pk2f *e)
{
    const pk2f ss = r.ur[0] * r.ur[0] + r.ur[1] * r.ur[1] + r.ur[2] * r.ur[2];
    pk2f inv;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (((r.pass >> j) & 1) && !(ss[j] >= SALSA_PK_FOA_MIN)) {
            r.pass &= ~(1 << j);
            r.unsure |= 1 << j;
        }
        float y = approx_rsqrtf(ss[j]);
        y = y * (1.5f - 0.5f * ss[j] * y * y); // one Newton step: the hardware seed is good to ~1 ulp already
        inv[j] = r.p00[j] < 0.f ? -y : y;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = r.ur[i] * inv;
}

// MIC feature of both frames: angle(sign(adj_00) u_i) / dk (normalise_mic_col0), float32 atan2.
SALSA_HD void normalise_mic_pk(pk_eig &r, float dk, pk2f *e)
{
    const float idk = 1.0f / dk;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const float sg = r.p00[j] < 0.f ? -1.f : 1.f;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float re = r.ur[i][j], im = r.ui[i][j];
            ok = ok && (re * re + im * im >= SALSA_PK_MIC_MIN);
            e[i][j] = atan2f(sg * im, sg * re) * idk;
        }
        if (((r.pass >> j) & 1) && !ok) {
            r.pass &= ~(1 << j);
            r.unsure |= 1 << j;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Stockham autosort FFT addressing, radix R, N points, N/R threads per transform.  Pass with sub-transform length p
// (p = 1, R, R^2, ... < N), thread i in [0, N/R), k = i & (p-1):
//   reads   x[i + r*(N/R)]                      r = 0..R-1
//   scales  element r by W_N^(r * k * N/(p*R))  (W_N = exp(-2 pi i / N))
//   writes  y[(i-k)*R + k + r*p]
// After the last pass y is the DFT in natural order.
SALSA_HD int stockham_in(int i, int r, int N, int R) { return i + r * (N / R); }
SALSA_HD int stockham_tw(int i, int r, int p, int N, int R) { return r * (i & (p - 1)) * (N / (p * R)); }
SALSA_HD int stockham_out(int i, int r, int p, int R) { int k = i & (p - 1); return (i - k) * R + k + r * p; }

// ---------------------------------------------------------------------------------------------------------------
// Noise-floor tracker step (salsa_feature_extraction.py:65-87).  Returns indicator_sig.
// Written so the dependent chain per frame is  multiply -> select -> max : both candidate products are formed before
// the above/below compare resolves.  Same operations and constants as the reference: floor_up = 1+alpha,
// floor_up_slow = 1+slow_scale*alpha, floor_down = 1-alpha (:31-35); "countdown -= 1; negative = countdown < 0" (:68-69)
// is (cd < 1) on the value before the decrement; the 1e-6 clamp (:85) is an fmax (the floor is never NaN).
template <bool CLAMP = true>
SALSA_HD bool tracker_step(double &floor, int &countdown, double mag, double snr_ratio = 1.5)
{
    const double up = (countdown < 1) ? 1.0 + 0.1 * 0.02 : 1.0 + 0.02;
    double pa = up * floor, pb = (1.0 - 0.02) * floor;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(pa), "+v"(pb)); // keep TWO products: the compiler would otherwise select the factor first and
                                           // put compare -> select -> multiply back on the dependent chain
#endif
    const bool above = mag > floor;
    countdown = above ? countdown - 1 : 3;
    const double sel = above ? pa : pb;
    if (CLAMP) {
#if defined(__HIP_DEVICE_COMPILE__)
        // one v_max_f64: fmax() would first canonicalise its operand (a second v_max on the dependent chain); sel is a
        // product of finite numbers, never a signalling NaN
        const double lim = 1e-6;
        asm("v_max_f64 %0, %1, %2" : "=v"(floor) : "v"(sel), "v"(lim));
#else
        floor = fmax(sel, 1e-6);
#endif
    } else {
        // CLAMP = false: the caller guarantees (by checking the minimum afterwards and redoing the block with CLAMP = true if it
        // fails) that sel >= 1e-6, where max(sel, 1e-6) == sel bit for bit: the clamp's float64 latency leaves the chain
        floor = sel;
    }
    return mag > snr_ratio * floor; // :87 (snr_ratio = 1.5 there; contrib's floor_mask_ratio kwarg)
}

// ---------------------------------------------------------------------------------------------------------------
// N x N Hermitian eigen-solver of the contrib surface at 5 - 16 microphones (cov_eig_n_kernel; contrib/salsa_flexible.py
// stacked_covmat_eigh :52-77 + the coherence test :353): cyclic complex Jacobi in float64 with the rotations accumulated
// (eigenvalues = the diagonal, eigenvectors = the accumulated columns).
// NCH > 0: compile-time size, fully unrolled (6 | 8).  NCH == 0: any even count up to HERMN_MAX read at run time -- the same code
// with run-time loop bounds and dynamically indexed arrays.
constexpr int HERMN_MAX = 16; // include/salsa_hip.h SALSA_MAX_MICS
constexpr int HERMN_SWEEPS = 16;
template <int NCH> struct hermn {
    static constexpr int S = NCH > 0 ? NCH : HERMN_MAX;
    double ar[S][S], ai[S][S];
};

template <int NCH>
SALSA_HD void hermn_rotate(hermn<NCH> &A, hermn<NCH> &V, const int p, const int q, const int n)
{
    const double xr = A.ar[p][q], xi = A.ai[p][q];
    const double r2 = xr * xr + xi * xi;
    if (r2 == 0.0) return;
    const double r = sqrt(r2);
    // a_pq = r e^{i phi}.  U = D G: D_qq = e^{-i phi} makes the pivot real, G is the real Jacobi rotation that zeroes it.
    const double er = xr / r, ei = xi / r;
    const double tau = (A.ar[q][q] - A.ar[p][p]) / (2.0 * r);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
    // U_pp = c, U_qp = -sn e^{-i phi}, U_pq = sn, U_qq = c e^{-i phi}
    const double uqp_r = -sn * er, uqp_i = sn * ei, uqq_r = c * er, uqq_i = -c * ei;
    auto cols = [&](hermn<NCH> &M) { // M <- M U (columns p and q)
#pragma unroll
        for (int i = 0; i < n; i++) {
            const double pr = M.ar[i][p], pi = M.ai[i][p], qr = M.ar[i][q], qi = M.ai[i][q];
            M.ar[i][p] = pr * c + (qr * uqp_r - qi * uqp_i);
            M.ai[i][p] = pi * c + (qr * uqp_i + qi * uqp_r);
            M.ar[i][q] = pr * sn + (qr * uqq_r - qi * uqq_i);
            M.ai[i][q] = pi * sn + (qr * uqq_i + qi * uqq_r);
        }
    };
    cols(A);
#pragma unroll
    for (int j = 0; j < n; j++) { // A <- U^H A (rows p and q): conj(U_pp) = c, conj(U_qp), conj(U_pq) = sn, conj(U_qq)
        const double pr = A.ar[p][j], pi = A.ai[p][j], qr = A.ar[q][j], qi = A.ai[q][j];
        A.ar[p][j] = c * pr + (uqp_r * qr + uqp_i * qi);
        A.ai[p][j] = c * pi + (uqp_r * qi - uqp_i * qr);
        A.ar[q][j] = sn * pr + (uqq_r * qr + uqq_i * qi);
        A.ai[q][j] = sn * pi + (uqq_r * qi - uqq_i * qr);
    }
    A.ar[p][q] = A.ai[p][q] = A.ar[q][p] = A.ai[q][p] = 0.0; // exactly, as the algebra says
    A.ai[p][p] = A.ai[q][q] = 0.0;
    cols(V);
}

// The per-bin solve of cov_eig_n_kernel on the summed covariance A (V = I on entry; both are left as the sweeps leave them:
// diag(A) = the eigenvalues, unsorted): the sweeps, the pick of the two largest eigenvalues, the gate
// "largest > second largest * ew_thresh" (:353) and, where it passes, the top eigenvector (ur, ui).  Returns the gate decision;
// `sweeps` = the number of sweeps run (HERMN_SWEEPS: left by the cap, not by the stop rule).
template <int NCH>
SALSA_HD bool hermn_gate_eigvec(hermn<NCH> &A, hermn<NCH> &V, const int n, const double cond, double *ur, double *ui, int &sweeps)
{
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < n; i++) tr += A.ar[i][i];
    bool good = false;
    sweeps = 0;
    if (tr > 0.0) {
        for (int sweep = 0; sweep < HERMN_SWEEPS; sweep++) {
            double off = 0.0;
#pragma unroll
            for (int p = 0; p < n; p++)
#pragma unroll
                for (int q = p + 1; q < n; q++) off += A.ar[p][q] * A.ar[p][q] + A.ai[p][q] * A.ai[p][q];
            if (off <= 1e-34 * tr * tr) break;
#pragma unroll
            for (int p = 0; p < n; p++)
#pragma unroll
                for (int q = p + 1; q < n; q++) hermn_rotate<NCH>(A, V, p, q, n);
            sweeps = sweep + 1;
        }
        int i1 = 0;
        double l1 = A.ar[0][0];
#pragma unroll
        for (int i = 1; i < n; i++)
            if (A.ar[i][i] > l1) { l1 = A.ar[i][i]; i1 = i; }
        double l2 = -1e300;
#pragma unroll
        for (int i = 0; i < n; i++)
            if (i != i1 && A.ar[i][i] > l2) l2 = A.ar[i][i];
        good = l1 > l2 * cond; // ews[:, -1] > ews[:, -2] * ew_thresh (:353)
        if (good) {
#pragma unroll
            for (int i = 0; i < n; i++) {
                ur[i] = ui[i] = 0.0;
#pragma unroll
                for (int j = 0; j < n; j++)
                    if (j == i1) { ur[i] = V.ar[i][j]; ui[i] = V.ai[i][j]; }
            }
        }
    }
    return good;
}

} // namespace salsa
