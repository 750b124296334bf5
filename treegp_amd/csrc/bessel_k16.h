// Derivative of the von Karman covariance profile in fp64.  With f(u) = u^(5/6) K_{5/6}(2 pi u) / lim0 (bessel_k56.h) and
// d/dx [x^nu K_nu(x)] = -x^nu K_{nu-1}(x) (A&S 9.6.28), f'(u) = -2 pi u^(5/6) K_{1/6}(2 pi u) / lim0.  What a gradient needs is
//     w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0,   u > 0
// because d f(u(x)) / dx = f'(u) du/dx and u du/dx is a polynomial in the coordinates (u^2 is the quadratic form).
// w grows like u^(-1/3) towards 0 (f has a cusp there: 1 - D u^(5/3)); the caller never asks for w(0) -- a pair at zero
// distance contributes no slope.  Finite for every finite u > 0, exactly 0 where bessel_k56.h returns exactly 0, NaN for NaN.
//
// Same scheme as bessel_k56.h for the single order 1/6 (published formulas restated):
//   x = 2 pi u <= 1 : K_{1/6} = pi (I_{-1/6} - I_{1/6}), ascending series (A&S 9.6.2 / 9.6.10).  With t = pi^2 u^2,
//                     w = C1 u^(-1/3) A(t) - C2 B(t): the powers of u fold into one cbrt.
//   x > 1           : g(x) = e^x sqrt(x) K_{1/6}(x) by piecewise Chebyshev (Clenshaw), tables from gen_bessel_k16_table.py;
//                     w = PRE u^(-2/3) exp(-x) g(x).
//   x > K56_XMAX    : 0 (the value's cutoff; w is still a normal number just below it).
// Host-compilable (tests build it with g++ and compare against mpmath).
#pragma once
#include "bessel_k56.h"
#include "bessel_k16_coeffs.h"

// `cheb`: where the 6 x K16_NDEG Chebyshev table is read from (an LDS copy on the device, see bessel_k56.h)
__host__ __device__ __forceinline__ double vonkarman_slope_tab(double u, const double *cheb) {
    const double x = K56_TWO_PI * u;
    if (x <= 1.0) {
        const double t = K56_PI2 * u * u;
        double sa = k16_sa[K16_NSER - 1], sb = k16_sb[K16_NSER - 1];
#pragma unroll
        for (int k = K16_NSER - 2; k >= 0; --k) {
            sa = fma(sa, t, k16_sa[k]);
            sb = fma(sb, t, k16_sb[k]);
        }
        return (K16_C1 / cbrt(u)) * sa - K16_C2 * sb;
    }
    if (!(x <= K56_XMAX)) return (x != x) ? x : 0.0;
    int e;
    (void)frexp(x, &e);                       // x in [2^(e-1), 2^e), e >= 1
    int idx = e - 1;
    double z;
    if (idx < 5) {
        z = ldexp(x, 1 - idx) - 3.0;          // 2 x / 2^idx - 3  in [-1, 1)
    } else {
        idx = 5;
        z = 64.0 / x - 1.0;                   // (-1, 1]
    }
    const double *c = cheb + idx * K16_NDEG;
    const double z2 = z + z;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = K16_NDEG - 1; k >= 1; --k) {
        const double b0 = fma(z2, b1, c[k]) - b2;
        b2 = b1;
        b1 = b0;
    }
    const double g = fma(z, b1, c[0]) - b2;
    const double cr = cbrt(u);
    return (K16_PRE / (cr * cr)) * exp(-x) * g;
}

__host__ __device__ __forceinline__ double vonkarman_slope(double u) { return vonkarman_slope_tab(u, &k16_cheb[0][0]); }

#ifdef __HIPCC__
// copy the table into `lds` (6 * K16_NDEG doubles); the caller synchronises the workgroup afterwards
__device__ __forceinline__ void vonkarman_slope_stage_table(double *lds) {
    for (int i = threadIdx.x; i < 6 * K16_NDEG; i += blockDim.x) lds[i] = (&k16_cheb[0][0])[i];
}
#endif
