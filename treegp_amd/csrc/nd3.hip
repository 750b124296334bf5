// Three-dimensional coordinates (seams S1, S2, S3 "in three dimensions" of include/tgp.h): every launch that EVALUATES a
// covariance for X in (n, 3) row-major.  What follows the K build does not know the dimension -- factorisation, sweeps, the kept
// factor and the posterior's substitution and products are the 2-D entries' launches (api.hip, cov.hip call the launchers here
// where their namesakes call kbuild.hip / predict.hip / cov.hip's own).
//   kbuild_slab3_kernel       the packed lower panels of kbuild_slab_kernel (64-row slabs of 256-wide panels, ld 256, identity
//                             padding, exact diagonal amp + yerr_i^2)
//   kernel_dense3_kernel      dense (n, m) matrix, self: diagonal exactly amp
//   cross_panels3_kernel      k(Xs, X) / k(Xs, Xs) in the zero-padded panels the posterior substitutes in
//   predict_partial3_kernel   fused mean, the decomposition of predict_partial_kernel (256 training points per LDS tile, partial
//   predict_gauss_tab3_kernel sums per split, fixed-order reduce); Gaussian kinds through coordinates transformed once per call
//   predict_grad_partial3_kernel   its gradient, three accumulators per query
// The bodies are written separately from the 2-D ones: the 2-D instantiations keep their arithmetic bit for bit.
// Arithmetic of a pair (d = the coordinate difference, taken first):
//   q = xx dx dx + 2xy dx dy + 2xz dx dz + yy dy dy + 2yz dy dz + zz dz dz      six products, the off-diagonals doubled on the host
//   Gaussian: amp exp(-q / 2);  von Karman: amp f(sqrt(q));  isotropic von Karman: amp f(sqrt(dx dx + dy dy + dz dz) / ell)
// with the amplitude multiplied after the transcendental.  q == 0 gives exactly amp; NaN stays NaN (exp, sqrt and bessel_k56.h
// pass it on; tgp_exp2_neg and exp2_neg_tab3 are written to).
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "bessel_k16.h"
#include "post_tile.h"

namespace {
constexpr int PT = 256;   // training points per LDS tile

struct K3Params {
    double amp, xx, xy2, xz2, yy, yz2, zz, inv_ell;
};

K3Params make_k3params(const tgp_kernel3 *k) {
    K3Params p;
    p.amp = k->amp;
    p.xx = k->m[0]; p.xy2 = 2.0 * k->m[1]; p.xz2 = 2.0 * k->m[2];
    p.yy = k->m[3]; p.yz2 = 2.0 * k->m[4]; p.zz = k->m[5];
    p.inv_ell = (k->ell != 0.0) ? 1.0 / k->ell : 0.0;
    return p;
}

__device__ __forceinline__ double quad_form3(const K3Params &p, double dx, double dy, double dz) {
    return p.xx * dx * dx + p.xy2 * dx * dy + p.xz2 * dx * dz + p.yy * dy * dy + p.yz2 * dy * dz + p.zz * dz * dz;
}

// amp k with the von Karman Chebyshev table read from `tab` (an LDS copy, bessel_k56.h); tab is ignored for Gaussians
template <int KE>
__device__ __forceinline__ double kernel_value3(const K3Params &p, double dx, double dy, double dz, const double *tab) {
    if constexpr (KE == KE_GAUSS) return p.amp * exp(-0.5 * quad_form3(p, dx, dy, dz));
    else if constexpr (KE == KE_VK) return p.amp * vonkarman_unit_tab(sqrt(dx * dx + dy * dy + dz * dz) * p.inv_ell, tab);
    else return p.amp * vonkarman_unit_tab(sqrt(quad_form3(p, dx, dy, dz)), tab);
}

// the K build's value: Gaussians take p.xx .. p.zz pre-scaled by 0.5 log2 e (launch_kbuild_lower3) and 2^-s from tgp_exp2_neg
template <int KE>
__device__ __forceinline__ double kb_value3(const K3Params &p, double dx, double dy, double dz, const double *tab) {
    if constexpr (KE == KE_GAUSS) return p.amp * tgp_exp2_neg(quad_form3(p, dx, dy, dz));
    else return kernel_value3<KE>(p, dx, dy, dz, tab);
}

// ---- K build: kbuild_slab_kernel with three coordinates ----------------------------------------------------------------------
// One workgroup = 64 consecutive rows of one 256-wide panel = one contiguous 128 KiB piece of the packed matrix.  Lane l owns
// columns 2l, 2l+1, 128+2l, 128+2l+1 of the panel (coordinates in registers), wave w rows w, w + 4, ... (coordinates wave-uniform).
template <int KE>
__global__ __launch_bounds__(256) void kbuild_slab3_kernel(K3Params p, const double *__restrict__ X, int64_t n, int64_t Np,
                                                           const double *__restrict__ yerr, double *__restrict__ A) {
    constexpr int SR = 64;
    __shared__ double vk_tab[KE == KE_GAUSS ? 1 : 6 * K56_NDEG];
    if constexpr (KE != KE_GAUSS) {
        vonkarman_stage_table(vk_tab);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // slabs before panel q: 4 (q P - q (q - 1) / 2) with P panels in all
    const int64_t b = blockIdx.x, P = Np / TGP_PW;
    const double B2 = 4.0 * P + 2.0;
    int64_t pj = (int64_t)((B2 - sqrt(B2 * B2 - 8.0 * (double)b)) * 0.25);
    if (pj < 0) pj = 0;
    if (pj > P - 1) pj = P - 1;
    while (pj > 0 && 4 * (pj * P - pj * (pj - 1) / 2) > b) --pj;
    while (pj + 1 < P && 4 * ((pj + 1) * P - (pj + 1) * pj / 2) <= b) ++pj;
    const int64_t slab = b - 4 * (pj * P - pj * (pj - 1) / 2);
    const int64_t i0 = pj * TGP_PW + slab * SR;              // first global row of the slab
    double *dst = A + panel_off(pj, Np) + slab * SR * TGP_PW + 2 * lane;

    int64_t jc[2] = {pj * TGP_PW + 2 * lane, pj * TGP_PW + TGP_TB + 2 * lane};
    double xj[2][2], yj[2][2], zj[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t j = jc[h] + e;
            xj[h][e] = j < n ? X[3 * j] : 0.0;
            yj[h][e] = j < n ? X[3 * j + 1] : 0.0;
            zj[h][e] = j < n ? X[3 * j + 2] : 0.0;
        }
    const bool diag_slab = slab < TGP_PW / SR;                // rows inside the panel's 256 x 256 diagonal block
    const bool upper_half_skip = slab < TGP_TB / SR;          // first 128 rows: the second tile lies above the diagonal
    const bool pad_slab = (i0 + SR > n) || (pj * TGP_PW + TGP_PW > n);

#pragma unroll 2
    for (int r = wave; r < SR; r += 4) {
        const int64_t i = i0 + r;
        double2 v[2];
        if (!pad_slab || i < n) {
            const int64_t ic = i < n ? i : 0;
            const double xi = X[3 * ic], yi = X[3 * ic + 1], zi = X[3 * ic + 2];   // wave-uniform
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v[h].x = kb_value3<KE>(p, xi - xj[h][0], yi - yj[h][0], zi - zj[h][0], vk_tab);
                v[h].y = kb_value3<KE>(p, xi - xj[h][1], yi - yj[h][1], zi - zj[h][1], vk_tab);
            }
            if (diag_slab) {
                // exact diagonal + noise
                const double e = yerr ? yerr[ic] : 0.0;
                const double d = p.amp + e * e;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (i == jc[h]) v[h].x = d;
                    if (i == jc[h] + 1) v[h].y = d;
                }
            }
            if (pad_slab) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (jc[h] >= n) v[h].x = 0.0;
                    if (jc[h] + 1 >= n) v[h].y = 0.0;
                }
            }
        } else {
            // padded rows: identity, so the padded factor is [[L, 0], [0, I]]
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v[h].x = (i == jc[h]) ? 1.0 : 0.0;
                v[h].y = (i == jc[h] + 1) ? 1.0 : 0.0;
            }
        }
        *reinterpret_cast<double2 *>(dst + (int64_t)r * TGP_PW) = v[0];
        if (!upper_half_skip) *reinterpret_cast<double2 *>(dst + (int64_t)r * TGP_PW + TGP_TB) = v[1];
    }
}

// ---- dense out[i*m + j] = amp k(X_i, Y_j); self != 0: Y == X and the diagonal is exactly amp ----------------------------------
template <int KE>
__global__ __launch_bounds__(256) void kernel_dense3_kernel(K3Params p, const double *__restrict__ X, int64_t n,
                                                            const double *__restrict__ Y, int64_t m, int self,
                                                            double *__restrict__ out) {
    __shared__ double vk_tab[KE == KE_GAUSS ? 1 : 6 * K56_NDEG];
    if constexpr (KE != KE_GAUSS) {
        vonkarman_stage_table(vk_tab);
        __syncthreads();
    }
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * 16;
    if (j >= m) return;
    const double xj = Y[3 * j], yj = Y[3 * j + 1], zj = Y[3 * j + 2];
    for (int r = 0; r < 16; ++r) {
        const int64_t i = i0 + r;
        if (i >= n) break;
        double v = kernel_value3<KE>(p, X[3 * i] - xj, X[3 * i + 1] - yj, X[3 * i + 2] - zj, vk_tab);
        if (self && i == j) v = p.amp;
        out[i * m + j] = v;
    }
}

// ---- cross panels of the posterior: out (rows x ncols in 256-column panels) = k(xs_i, x_j) for i < m, j < n, 0 outside ----------
template <int KE>
__global__ __launch_bounds__(256) void cross_panels3_kernel(K3Params p, const double *__restrict__ Xs, int64_t m,
                                                            const double *__restrict__ X, int64_t n, int self,
                                                            double *__restrict__ out, int64_t rows, int64_t ncols) {
    __shared__ double vk_tab[KE == KE_GAUSS ? 1 : 6 * K56_NDEG];
    if constexpr (KE != KE_GAUSS) {
        vonkarman_stage_table(vk_tab);
        __syncthreads();
    }
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= ncols) return;
    double v = 0.0;
    if (i < m && j < n) {
        v = kernel_value3<KE>(p, Xs[3 * i] - X[3 * j], Xs[3 * i + 1] - X[3 * j + 1], Xs[3 * i + 2] - X[3 * j + 2], vk_tab);
        if (self && i == j) v = p.amp;
    }
    out[panel_elem(i, j, rows)] = v;
}

// ---- fused mean ---------------------------------------------------------------------------------------------------------------
// One thread per query point; the training points (x, y, z, alpha) go through LDS in tiles of 256 and come back as wave-wide
// broadcasts.  The training set is split over gridDim.y; the partial sums are combined in a fixed order by predict_reduce3_kernel.
template <int KE>
__global__ __launch_bounds__(256) void predict_partial3_kernel(K3Params p, const double *__restrict__ X, int64_t n,
                                                               const double *__restrict__ alpha, const double *__restrict__ Xs,
                                                               int64_t m, double *__restrict__ partial, int64_t chunk) {
    __shared__ double sx[PT], sy[PT], sz[PT], sa[PT];
    __shared__ double vk_tab[KE == KE_GAUSS ? 1 : 6 * K56_NDEG];
    if constexpr (KE != KE_GAUSS) vonkarman_stage_table(vk_tab);       // (the first barrier of the loop below publishes it)
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * 256 + tid;
    const int64_t i_begin = (int64_t)blockIdx.y * chunk;
    const int64_t i_end = (i_begin + chunk < n) ? i_begin + chunk : n;
    double xq = 0.0, yq = 0.0, zq = 0.0;
    if (q < m) { xq = Xs[3 * q]; yq = Xs[3 * q + 1]; zq = Xs[3 * q + 2]; }
    double acc = 0.0;
    for (int64_t i0 = i_begin; i0 < i_end; i0 += PT) {
        const int64_t i = i0 + tid;
        __syncthreads();
        if (i < i_end) { sx[tid] = X[3 * i]; sy[tid] = X[3 * i + 1]; sz[tid] = X[3 * i + 2]; sa[tid] = alpha[i]; }
        else { sx[tid] = 0.0; sy[tid] = 0.0; sz[tid] = 0.0; sa[tid] = 0.0; }
        __syncthreads();
        const int cnt = (int)((i_end - i0 < PT) ? (i_end - i0) : PT);
        if (cnt == PT) {
#pragma unroll 4
            for (int t = 0; t < PT; ++t) acc += kernel_value3<KE>(p, xq - sx[t], yq - sy[t], zq - sz[t], vk_tab) * sa[t];
        } else {
            for (int t = 0; t < cnt; ++t) acc += kernel_value3<KE>(p, xq - sx[t], yq - sy[t], zq - sz[t], vk_tab) * sa[t];
        }
    }
    if (q < m) partial[(int64_t)blockIdx.y * m + q] = acc;
}

// Gaussian fast path, as predict_gauss_tab_kernel: exp(-0.5 d^T invLam d) with invLam = L L^T (3 x 3 Cholesky) is
// 2^-(|u|^2 / 256) for u = sqrt(0.5 log2 e 256) L^T d.  The coordinates are transformed once per call, relative to the first
// training point (subtracted BEFORE the transform: exact for data whose spread is small against its offset), which leaves
// 3 sub + 1 mul + 2 fma for the exponent.  The amplitude is applied in the reduction.
__global__ __launch_bounds__(256) void predict_transform3_kernel(const double *__restrict__ X, int64_t n,
                                                                 const double *__restrict__ origin, double t00, double t10,
                                                                 double t20, double t11, double t21, double t22,
                                                                 double *__restrict__ U) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = X[3 * i] - origin[0], y = X[3 * i + 1] - origin[1], z = X[3 * i + 2] - origin[2];
    U[3 * i] = t00 * x + t10 * y + t20 * z;
    U[3 * i + 1] = t11 * y + t21 * z;
    U[3 * i + 2] = t22 * z;
}

// 2^(-w / 256), w >= 0: 2^t = 2^e 2^(j/256) 2^(r/256) with t 256 = e 256 + j + r, |r| <= 1/2; 2^(j/256) from the 256-entry table
// (correctly rounded), 2^(r/256) from a degree-4 Taylor polynomial (remainder 5e-17 relative): <= 1.5 ulp with the product.
// The arithmetic of predict.hip's exp2_neg_tab<256>, restated.  A NaN w gives NaN (the polynomial carries it; the conversion of
// NaN to int is 0).  Huge w: the conversion saturates and ldexp(., -2^23) is 0.
__device__ __forceinline__ double exp2_neg_tab3(double w, const double *tab) {
    constexpr double L = 0.69314718055994530942 / 256;
    const double t = -w;
    const double k = rint(t);
    const double r = t - k;                                    // exact, |r| <= 0.5
    double p = L * L * L * L / 24.0;
    p = fma(p, r, L * L * L / 6.0);
    p = fma(p, r, L * L / 2.0);
    p = fma(p, r, L);
    p = fma(p, r, 1.0);
    const int ki = (int)k;
    return ldexp(tab[ki & 255] * p, ki >> 8);
}

__global__ __launch_bounds__(256) void predict_gauss_tab3_kernel(const double *__restrict__ U, int64_t n,
                                                                 const double *__restrict__ alpha, const double *__restrict__ Us,
                                                                 int64_t m, const double *__restrict__ exp2_j256,
                                                                 double *__restrict__ partial, int64_t chunk) {
    __shared__ double sx[PT], sy[PT], sz[PT], sa[PT];
    __shared__ double tab[256];
    const int tid = threadIdx.x;
    tab[tid] = exp2_j256[tid];                                         // (the first barrier of the loop below publishes it)
    const int64_t q = (int64_t)blockIdx.x * 256 + tid;
    const int64_t i_begin = (int64_t)blockIdx.y * chunk;
    const int64_t i_end = (i_begin + chunk < n) ? i_begin + chunk : n;
    double xq = 0.0, yq = 0.0, zq = 0.0;
    if (q < m) { xq = Us[3 * q]; yq = Us[3 * q + 1]; zq = Us[3 * q + 2]; }
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t i0 = i_begin; i0 < i_end; i0 += PT) {
        const int64_t i = i0 + tid;
        __syncthreads();
        if (i < i_end) { sx[tid] = U[3 * i]; sy[tid] = U[3 * i + 1]; sz[tid] = U[3 * i + 2]; sa[tid] = alpha[i]; }
        else { sx[tid] = 0.0; sy[tid] = 0.0; sz[tid] = 0.0; sa[tid] = 0.0; }          // alpha = 0: padded entries add nothing
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < PT; t += 2) {
            const double dx0 = xq - sx[t], dy0 = yq - sy[t], dz0 = zq - sz[t];
            const double dx1 = xq - sx[t + 1], dy1 = yq - sy[t + 1], dz1 = zq - sz[t + 1];
            acc0 = fma(exp2_neg_tab3(fma(dx0, dx0, fma(dy0, dy0, dz0 * dz0)), tab), sa[t], acc0);
            acc1 = fma(exp2_neg_tab3(fma(dx1, dx1, fma(dy1, dy1, dz1 * dz1)), tab), sa[t + 1], acc1);
        }
    }
    if (q < m) partial[(int64_t)blockIdx.y * m + q] = acc0 + acc1;
}

__global__ __launch_bounds__(256) void predict_reduce3_kernel(const double *__restrict__ partial, int64_t m, int nsplit,
                                                              double scale, double *__restrict__ ys) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += partial[(int64_t)k * m + q];
    ys[q] = scale * s;
}

// ---- gradient of the mean: gs[q] = sum_i alpha_i amp grad_x k(x - X_i) at x = Xs_q -----------------------------------------------
// With d = Xs_q - X_i and M = invLam, grad k = -k M d (Gaussian) and -w(u) M d (von Karman, u^2 = d^T M d, w = -f'(u) / u from
// bessel_k16.h; the isotropic kind has M = I / ell^2).  A pair at u == 0 contributes exactly 0: M d = 0 there for the Gaussian
// kinds and the von Karman field has zero slope on a star (w is not evaluated).  Three accumulators per thread, their partial
// sums stored as three planes of m queries per split; the reduction applies -amp.
template <int KE>
__global__ __launch_bounds__(256) void predict_grad_partial3_kernel(K3Params p, const double *__restrict__ X, int64_t n,
                                                                    const double *__restrict__ alpha,
                                                                    const double *__restrict__ Xs, int64_t m,
                                                                    double *__restrict__ partial, int64_t chunk) {
    __shared__ double sx[PT], sy[PT], sz[PT], sa[PT];
    __shared__ double vk_tab[KE == KE_GAUSS ? 1 : 6 * K16_NDEG];
    if constexpr (KE != KE_GAUSS) vonkarman_slope_stage_table(vk_tab); // (the first barrier of the loop below publishes it)
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * 256 + tid;
    const int64_t i_begin = (int64_t)blockIdx.y * chunk;
    const int64_t i_end = (i_begin + chunk < n) ? i_begin + chunk : n;
    // M, symmetric; the isotropic von Karman kind keeps u = |d| / ell as the value does
    const double e2 = p.inv_ell * p.inv_ell;
    const double mxx = (KE == KE_VK) ? e2 : p.xx, mxy = (KE == KE_VK) ? 0.0 : 0.5 * p.xy2, mxz = (KE == KE_VK) ? 0.0 : 0.5 * p.xz2;
    const double myy = (KE == KE_VK) ? e2 : p.yy, myz = (KE == KE_VK) ? 0.0 : 0.5 * p.yz2, mzz = (KE == KE_VK) ? e2 : p.zz;
    double xq = 0.0, yq = 0.0, zq = 0.0;
    if (q < m) { xq = Xs[3 * q]; yq = Xs[3 * q + 1]; zq = Xs[3 * q + 2]; }
    double accx = 0.0, accy = 0.0, accz = 0.0;
    auto pair = [&](int t) {
        const double dx = xq - sx[t], dy = yq - sy[t], dz = zq - sz[t];
        const double gx = mxx * dx + mxy * dy + mxz * dz, gy = mxy * dx + myy * dy + myz * dz, gz = mxz * dx + myz * dy + mzz * dz;   // M d
        double s;
        if constexpr (KE == KE_GAUSS) {
            s = exp(-0.5 * (dx * gx + dy * gy + dz * gz)) * sa[t];
        } else {
            const double u = (KE == KE_VK) ? sqrt(dx * dx + dy * dy + dz * dz) * p.inv_ell : sqrt(dx * gx + dy * gy + dz * gz);
            s = (u == 0.0) ? 0.0 : vonkarman_slope_tab(u, vk_tab) * sa[t];
        }
        accx = fma(s, gx, accx);
        accy = fma(s, gy, accy);
        accz = fma(s, gz, accz);
    };
    for (int64_t i0 = i_begin; i0 < i_end; i0 += PT) {
        const int64_t i = i0 + tid;
        __syncthreads();
        if (i < i_end) { sx[tid] = X[3 * i]; sy[tid] = X[3 * i + 1]; sz[tid] = X[3 * i + 2]; sa[tid] = alpha[i]; }
        else { sx[tid] = 0.0; sy[tid] = 0.0; sz[tid] = 0.0; sa[tid] = 0.0; }
        __syncthreads();
        const int cnt = (int)((i_end - i0 < PT) ? (i_end - i0) : PT);
        if (cnt == PT) {
#pragma unroll 2
            for (int t = 0; t < PT; ++t) pair(t);
        } else {
            for (int t = 0; t < cnt; ++t) pair(t);
        }
    }
    if (q < m) {
        partial[((int64_t)blockIdx.y * 3) * m + q] = accx;
        partial[((int64_t)blockIdx.y * 3 + 1) * m + q] = accy;
        partial[((int64_t)blockIdx.y * 3 + 2) * m + q] = accz;
    }
}

__global__ __launch_bounds__(256) void predict_grad_reduce3_kernel(const double *__restrict__ partial, int64_t m, int nsplit,
                                                                   double scale, double *__restrict__ gs) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nsplit; ++k) {
        s0 += partial[((int64_t)k * 3) * m + q];
        s1 += partial[((int64_t)k * 3 + 1) * m + q];
        s2 += partial[((int64_t)k * 3 + 2) * m + q];
    }
    gs[3 * q] = scale * s0;
    gs[3 * q + 1] = scale * s1;
    gs[3 * q + 2] = scale * s2;
}
}  // namespace

int tgp_kernel3_check(tgp_ctx *ctx, const tgp_kernel3 *k, const char *fn) {
    if (!ctx) return -1;
    if (!k) { ctx->err = std::string(fn) + ": the kernel must not be NULL"; return -1; }
    if (k->ndim != 3) {
        ctx->err = std::string(fn) + ": tgp_kernel3.ndim = " + std::to_string(k->ndim) + " must be 3";
        return -1;
    }
    if (kind_to_ke(k->kind) < 0) {
        ctx->err = std::string(fn) + ": unknown kernel kind tgp_kernel3.kind = " + std::to_string(k->kind);
        return -1;
    }
    return 0;
}

#define TGP_LAUNCH3(KERNEL, GRID, ...)                                                                          \
    switch (kind_to_ke(k->kind)) {                                                                             \
        case KE_GAUSS: KERNEL<KE_GAUSS><<<GRID, 256, 0, ctx->stream>>>(__VA_ARGS__); break;                    \
        case KE_VK: KERNEL<KE_VK><<<GRID, 256, 0, ctx->stream>>>(__VA_ARGS__); break;                          \
        default: KERNEL<KE_AVK><<<GRID, 256, 0, ctx->stream>>>(__VA_ARGS__); break;                            \
    }

int launch_kbuild_lower3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_X, int64_t n, int64_t Np, const double *d_yerr,
                         double *d_A) {
    TGP_ARG(kind_to_ke(k->kind) >= 0 && n > 0 && Np % TGP_PW == 0 && n <= Np);
    K3Params p = make_k3params(k);
    if (kind_to_ke(k->kind) == KE_GAUSS) {
        const double c0 = 0.72134752044448170368;                            // 0.5 log2 e: exp(-q/2) = 2^-(c0 q)
        p.xx *= c0; p.xy2 *= c0; p.xz2 *= c0; p.yy *= c0; p.yz2 *= c0; p.zz *= c0;
    }
    const int64_t P = Np / TGP_PW;
    dim3 grid((unsigned)(4 * (P * (P + 1) / 2)));                            // 64-row slabs of all panels, in memory order
    TGP_LAUNCH3(kbuild_slab3_kernel, grid, p, d_X, n, Np, d_yerr, d_A)
    TGP_HIP(hipGetLastError());
    return 0;
}

int launch_kernel_dense3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_X, int64_t n, const double *d_Y, int64_t m, int self,
                         double *d_out) {
    TGP_ARG(kind_to_ke(k->kind) >= 0 && n > 0 && m > 0 && (n + 15) / 16 <= 65535);
    const K3Params p = make_k3params(k);
    dim3 grid((unsigned)((m + 255) / 256), (unsigned)((n + 15) / 16));
    TGP_LAUNCH3(kernel_dense3_kernel, grid, p, d_X, n, d_Y, m, self, d_out)
    TGP_HIP(hipGetLastError());
    return 0;
}

int launch_cross_panels3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_Xs, int64_t m, const double *d_X, int64_t n, int self,
                         double *d_out, int64_t rows, int64_t ncols) {
    TGP_ARG(kind_to_ke(k->kind) >= 0 && rows > 0 && rows <= 65535 && ncols > 0 && m <= rows && n <= ncols);
    const K3Params p = make_k3params(k);
    dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)rows);
    TGP_LAUNCH3(cross_panels3_kernel, grid, p, d_Xs, m, d_X, n, self, d_out, rows, ncols)
    TGP_HIP(hipGetLastError());
    return 0;
}

// invLam = L L^T, L lower triangular with a positive diagonal but for l22 >= 0; false when invLam has no such factor (rank
// deficient in its leading 2 x 2 block, indefinite, or NaN): the caller evaluates the quadratic form directly then
static bool cholesky3(const tgp_kernel3 *k, double l[6]) {
    const double xx = k->m[0], xy = k->m[1], xz = k->m[2], yy = k->m[3], yz = k->m[4], zz = k->m[5];
    if (!(xx > 0.0)) return false;
    const double l00 = sqrt(xx), l10 = xy / l00, l20 = xz / l00;
    const double d11 = yy - l10 * l10;
    if (!(d11 > 0.0)) return false;
    const double l11 = sqrt(d11), l21 = (yz - l20 * l10) / l11;
    const double d22 = zz - l20 * l20 - l21 * l21;
    if (!(d22 >= 0.0)) return false;
    l[0] = l00; l[1] = l10; l[2] = l20; l[3] = l11; l[4] = l21; l[5] = sqrt(d22);
    for (int i = 0; i < 6; ++i)
        if (!(l[i] - l[i] == 0.0)) return false;                              // an infinite entry
    return true;
}

int launch_predict3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_X, int64_t n, const double *d_alpha, const double *d_Xs,
                    int64_t m, double *d_ys) {
    const int ke = kind_to_ke(k->kind);
    TGP_ARG(ke >= 0);
    TGP_ARG(n > 0 && m > 0);
    const K3Params p = make_k3params(k);
    const int64_t qblocks = (m + 255) / 256;
    // the split of launch_predict: many more workgroups than slots, never finer than one LDS tile
    int64_t nsplit = (14336 + qblocks - 1) / qblocks;
    const int64_t maxsplit = (n + PT - 1) / PT;
    if (nsplit > maxsplit) nsplit = maxsplit;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 65535) nsplit = 65535;
    int64_t chunk = (n + nsplit - 1) / nsplit;
    chunk = (chunk + PT - 1) / PT * PT;
    nsplit = (n + chunk - 1) / chunk;
    int rc = tgp_ensure_scratch(ctx, rup((size_t)nsplit * m * 8) + rup(3 * n * 8) + rup(3 * m * 8) + rup(256 * 8));
    if (rc) return rc;
    double *partial = (double *)ctx->scratch;
    dim3 grid((unsigned)qblocks, (unsigned)nsplit);
    double l[6];
    if (ke == KE_GAUSS && cholesky3(k, l)) {
        const double sc = 0.84932180028801904272 * 16.0;                     // sqrt(0.5 log2 e 256)
        double *U = (double *)((char *)ctx->scratch + rup((size_t)nsplit * m * 8));
        double *Us = (double *)((char *)U + rup(3 * n * 8));
        double *d_tab = (double *)((char *)Us + rup(3 * m * 8));             // the 2^(j/256) table, copied per call (written before read)
        rc = launch_exp2_j256_copy(ctx, d_tab);
        if (rc) return rc;
        predict_transform3_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_X, n, d_X, sc * l[0], sc * l[1], sc * l[2],
                                                                                        sc * l[3], sc * l[4], sc * l[5], U);
        predict_transform3_kernel<<<(unsigned)((m + 255) / 256), 256, 0, ctx->stream>>>(d_Xs, m, d_X, sc * l[0], sc * l[1], sc * l[2],
                                                                                        sc * l[3], sc * l[4], sc * l[5], Us);
        predict_gauss_tab3_kernel<<<grid, 256, 0, ctx->stream>>>(U, n, d_alpha, Us, m, d_tab, partial, chunk);
        predict_reduce3_kernel<<<(unsigned)qblocks, 256, 0, ctx->stream>>>(partial, m, (int)nsplit, k->amp, d_ys);
        TGP_HIP(hipGetLastError());
        return 0;
    }
    TGP_LAUNCH3(predict_partial3_kernel, grid, p, d_X, n, d_alpha, d_Xs, m, partial, chunk)
    predict_reduce3_kernel<<<(unsigned)qblocks, 256, 0, ctx->stream>>>(partial, m, (int)nsplit, 1.0, d_ys);
    TGP_HIP(hipGetLastError());
    return 0;
}

// As launch_predict_grad: the split of the training set depends on n alone and the queries go through in slabs, so that a query's
// bits depend on nothing but the training set and its own coordinates.
int launch_predict_grad3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_X, int64_t n, const double *d_alpha,
                         const double *d_Xs, int64_t m, double *d_gs) {
    constexpr int64_t GRAD_SLAB = 32768, GRAD_MAXSPLIT = 128;
    TGP_ARG(kind_to_ke(k->kind) >= 0);
    TGP_ARG(n > 0 && m > 0);
    const K3Params p = make_k3params(k);
    int64_t nsplit = (n + PT - 1) / PT;
    if (nsplit > GRAD_MAXSPLIT) nsplit = GRAD_MAXSPLIT;
    int64_t chunk = (n + nsplit - 1) / nsplit;
    chunk = (chunk + PT - 1) / PT * PT;
    nsplit = (n + chunk - 1) / chunk;
    const int64_t slab = (m < GRAD_SLAB) ? m : GRAD_SLAB;
    int rc = tgp_ensure_scratch(ctx, rup((size_t)nsplit * 3 * slab * 8));
    if (rc) return rc;
    double *partial = (double *)ctx->scratch;
    for (int64_t q0 = 0; q0 < m; q0 += GRAD_SLAB) {
        const int64_t ms = (m - q0 < GRAD_SLAB) ? m - q0 : GRAD_SLAB;
        const unsigned qblocks = (unsigned)((ms + 255) / 256);
        dim3 grid(qblocks, (unsigned)nsplit);
        const double *xs = d_Xs + 3 * q0;
        TGP_LAUNCH3(predict_grad_partial3_kernel, grid, p, d_X, n, d_alpha, xs, ms, partial, chunk)
        predict_grad_reduce3_kernel<<<qblocks, 256, 0, ctx->stream>>>(partial, ms, (int)nsplit, -k->amp, d_gs + 3 * q0);
    }
    TGP_HIP(hipGetLastError());
    return 0;
}
