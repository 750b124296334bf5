// The device bodies of the posterior (S3b / S3c / S3f) and of the likelihood gradient (S2d / S2f), shared by cov.hip (one
// problem per launch) and batch.hip (the problem index on the grid).  The __global__ kernels of both files only decode
// blockIdx, apply their own early exits, offset the pointers to their problem and call these: every sum below has ONE
// order, whichever route runs it.
#pragma once
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "bessel_k16.h"
#include "gemm_tile.h"

// element (i, j) of a `rows`-row array stored in 256-column panels (panel p at p * rows * 256, ld 256)
__host__ __device__ inline int64_t panel_elem(int64_t i, int64_t j, int64_t rows) {
    return (j >> 8) * rows * TGP_PW + i * TGP_PW + (j & 255);
}

// k(xs_i, x_j) for i < m, j < n, 0 outside; `self`: x is xs and the diagonal is exactly amp
template <int KE>
__device__ __forceinline__ double cross_value(const KParams &p, const double *__restrict__ xs, int64_t m,
                                              const double *__restrict__ x, int64_t n, int self, int64_t i, int64_t j) {
    double v = 0.0;
    if (i < m && j < n) {
        v = kernel_value<KE>(p, xs[2 * i] - x[2 * j], xs[2 * i + 1] - x[2 * j + 1]);
        if (self && i == j) v = p.amp;
    }
    return v;
}

// Bk <- Bk W^T for one 128-row tile of column block kb (W = the inverse of the factor's diagonal block)
__device__ __forceinline__ void post_trsm_tile(double *Bk, const double *W) { gemm_tile_128<0, TGP_TB, TGP_TB>(Bk, W, Bk); }

// Bt[ti, c] -= Bt[ti, kb] L[c, kb]^T.  Bt holds the panels from pb on (panel p at Bt + (p - pb) * Mp * 256)
__device__ __forceinline__ void post_update_tile(double *Bt, int64_t Mp, const double *A, int64_t Np, int kb, int64_t pb, int64_t ti,
                                                 int64_t c) {
    const int64_t p = kb >> 1;
    const double *a = Bt + (p - pb) * Mp * TGP_PW + ti * TGP_TB * TGP_PW + (kb & 1) * TGP_TB;
    const double *b = A + panel_off(p, Np) + (c * TGP_TB - p * TGP_PW) * TGP_PW + (kb & 1) * TGP_TB;
    double *cc = Bt + ((c >> 1) - pb) * Mp * TGP_PW + ti * TGP_TB * TGP_PW + (c & 1) * TGP_TB;
    gemm_tile_dtv<4, TGP_TB, 1>(a, b, cc, nullptr, nullptr);
}

// C(ti, tj) -= sum over the panels p0 .. nP - 1 of Bt[ti] Bt[tj]^T (C in the same panel layout, Mp rows).  p0 = 0: the
// covariance; p0 = ti / 2: -K^-1 from Bt = L^-T, whose row tile ti is zero left of its own panel
__device__ __forceinline__ void post_syrk_tile(double *C, const double *Bt, int64_t Mp, int nP, int64_t ti, int64_t tj, int64_t p0) {
    const double *a = Bt + p0 * Mp * TGP_PW + ti * TGP_TB * TGP_PW;
    const double *b = Bt + p0 * Mp * TGP_PW + tj * TGP_TB * TGP_PW;
    double *c = C + (tj >> 1) * Mp * TGP_PW + ti * TGP_TB * TGP_PW + (tj & 1) * TGP_TB;
    gemm_tile_dtv<4, TGP_PW, 0>(a, b, c, nullptr, nullptr, nP - (int)p0, Mp * TGP_PW, Mp * TGP_PW);
}

// ---- diagonal blocks of (K + D)^-1 (seam S3h): [P]_ij = Bt_i . Bt_j over the rows of one group -----------------------------------
// One 128 x 128 tile pair of one group's block.  The items are laid out by the host (cov.hip: tgp_factor_inv_blocks); item q
// owns tile slot q of the staging buffer C: two slots side by side per 128 x 256 strip (ld 256), as the tiles of a panel.
struct InvBlockItem {
    int ta, tb;      // 128-row tiles of the chunk's Bt, ta >= tb
    int p0, nseg;    // first stored panel the sum covers (the one that holds the group's first row) and how many follow
    int ra, rb;      // row of the group's block that row 0 of tile ta / tb is (negative: the tile starts above the group)
    int g, pad;      // rows of the group
    int64_t out;     // where the group's g x g block starts in the chunk's output
};
__device__ __forceinline__ double *inv_block_slot(double *C, int64_t q) {
    return C + (q >> 1) * TGP_TB * TGP_PW + (q & 1) * TGP_TB;
}
// slot q of C (zero before) <- -sum over the panels p0 .. p0 + nseg - 1 of Bt[ta] Bt[tb]^T: post_syrk_tile's product, with ONE
// first panel for every pair of a group, so that an entry's sum has the same terms in the same order wherever the group lies
// in its chunk
__device__ __forceinline__ void inv_block_syrk_tile(double *C, const double *Bt, int64_t Mp, const InvBlockItem *items, int64_t q) {
    const int ta = __builtin_amdgcn_readfirstlane(items[q].ta), tb = __builtin_amdgcn_readfirstlane(items[q].tb);
    const int p0 = __builtin_amdgcn_readfirstlane(items[q].p0), nseg = __builtin_amdgcn_readfirstlane(items[q].nseg);
    const double *a = Bt + (int64_t)p0 * Mp * TGP_PW + (int64_t)ta * TGP_TB * TGP_PW;
    const double *b = Bt + (int64_t)p0 * Mp * TGP_PW + (int64_t)tb * TGP_TB * TGP_PW;
    gemm_tile_dtv<4, TGP_PW, 0>(a, b, inv_block_slot(C, q), nullptr, nullptr, nseg, Mp * TGP_PW, Mp * TGP_PW);
}
// the entries of slot q that belong to the group, negated (exact), into its row-major block: the lower triangle as computed
// and its mirror image, so both halves carry the same bits.  Rows and columns of the tiles outside the group are dropped.
// Every entry of the block is written by exactly one thread of one item: no atomics.
__device__ __forceinline__ void inv_block_write_tile(const double *C, const InvBlockItem *items, int64_t q, double *out) {
    const InvBlockItem it = items[q];
    const double *c = inv_block_slot(const_cast<double *>(C), q);
    double *blk = out + it.out;
    for (int idx = threadIdx.x; idx < TGP_TB * TGP_TB; idx += 256) {
        const int r = idx >> 7, col = idx & 127;
        const int i = it.ra + r, j = it.rb + col;
        if (i < 0 || i >= it.g || j < 0 || j > i) continue;
        const double v = -c[r * TGP_PW + col];
        blk[(int64_t)i * it.g + j] = v;
        if (i != j) blk[(int64_t)j * it.g + i] = v;
    }
}

// |Bt[i, :]|^2 over nP panels by one wave: each lane squares 2 + 2 doubles of every 256-wide panel row (two 16-byte loads,
// 1 KiB contiguous per wave and load), lane partials run over the panels in order, then a fixed xor tree across the wave.
// No atomics.  Every lane returns the sum.
__device__ __forceinline__ double row_sqnorm_wave(const double *__restrict__ Bt, int64_t Mp, int nP, int64_t i) {
    const int lane = threadIdx.x & 63;
    const double *row = Bt + i * TGP_PW + 2 * lane;
    double acc = 0.0;
#pragma unroll 4
    for (int p = 0; p < nP; ++p) {
        const double2 a = *(const double2 *)(row + (int64_t)p * Mp * TGP_PW);
        const double2 b = *(const double2 *)(row + (int64_t)p * Mp * TGP_PW + 128);
        acc += (a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// The same over the panels p0 .. nP - 1 only, for a row that is zero (or was never written) left of panel p0: row i of
// Bt = L^-T with p0 = (i / 128) / 2, whose squared norm is [K^-1]_ii.  Same loads and the same order (panels in order from p0,
// then the xor tree); the products are spelled out as fma so that every trip of the loop, unrolled or not, rounds alike:
// trailing panels of exact zeros add nothing, whatever nP is.  No atomics.  Every lane returns the sum.
__device__ __forceinline__ double row_sqnorm_wave_from(const double *__restrict__ Bt, int64_t Mp, int nP, int64_t i, int p0) {
    const int lane = threadIdx.x & 63;
    const double *row = Bt + i * TGP_PW + 2 * lane;
    double acc = 0.0;
#pragma unroll 4
    for (int p = p0; p < nP; ++p) {
        const double2 a = *(const double2 *)(row + (int64_t)p * Mp * TGP_PW);
        const double2 b = *(const double2 *)(row + (int64_t)p * Mp * TGP_PW + 128);
        acc += fma(a.y, a.y, a.x * a.x) + fma(b.y, b.y, b.x * b.x);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// The likelihood gradient's pair sum of one workgroup: rows i0 .. i0 + 63 x the 256-column panel pj of the lower triangle
// below n, against C = -K^-1 (panels of Mp rows); the four partial sums to out[0 .. 3].
// KE_GAUSS: dK/d(a, b, c) = -1/2 K (dx^2, 2 dx dy, dy^2).  KE_VK / KE_AVK (seam S2h): K = amp f(u), u^2 the quadratic form, so
// dK/d(a, b, c) = amp f'(u) / (2 u) (dx^2, 2 dx dy, dy^2) = -1/2 amp w(u) (...) with w = -f'/u of bessel_k16.h: the Gaussian
// body with f in slot 0 and w in slots 1 .. 3, both from one u, evaluated as the value kernel evaluates it.  A pair at u == 0
// off the diagonal counts f = 1 and no slope (w(0) is infinite and is never asked for); beyond the value's cutoff both are 0.
// The von Karman kinds read both Chebyshev tables from LDS copies made once per workgroup.  `p.kind` is not read.
template <int KE>
__device__ __forceinline__ void loglik_grad_block(const KParams &p, const double *__restrict__ X, const double *__restrict__ alpha,
                                                  const double *__restrict__ Cpm, int64_t Mp, int64_t n, int64_t pj, int64_t i0,
                                                  double *__restrict__ out) {
    __shared__ double red[4][4];
    __shared__ double tab_f[KE == KE_GAUSS ? 1 : 6 * K56_NDEG], tab_w[KE == KE_GAUSS ? 1 : 6 * K16_NDEG];
    if constexpr (KE != KE_GAUSS) {
        vonkarman_stage_table(tab_f);
        vonkarman_slope_stage_table(tab_w);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const int64_t j = pj * TGP_PW + tid;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (pj * TGP_PW <= i0 + 63 && j < n) {
        const double xj = X[2 * j], yj = X[2 * j + 1], aj = alpha[j];
        const double *col = Cpm + pj * Mp * TGP_PW + tid;
        for (int r = 0; r < 64; ++r) {
            const int64_t i = i0 + r;
            if (i >= n) break;
            if (j > i) continue;
            const double m = alpha[i] * aj + col[i * TGP_PW];       // alpha_i alpha_j - [K^-1]_ij   (C holds -K^-1)
            if (i == j) {
                acc[0] += 0.5 * m * p.amp;                          // the pair (i, i) counts once, d K_ii / d log amp = amp
            } else {
                const double dx = X[2 * i] - xj, dy = X[2 * i + 1] - yj;
                if constexpr (KE == KE_GAUSS) {
                    const double e = p.amp * exp(-0.5 * quad_form(p, dx, dy)) * m;
                    acc[0] += e;
                    acc[1] -= 0.5 * e * dx * dx;
                    acc[2] -= e * dx * dy;
                    acc[3] -= 0.5 * e * dy * dy;
                } else {
                    const double u = (KE == KE_VK) ? sqrt(dx * dx + dy * dy) * p.inv_ell : sqrt(quad_form(p, dx, dy));
                    if (u == 0.0) {
                        acc[0] += p.amp * m;                        // coincident points: f = 1, no slope
                    } else {
                        acc[0] += p.amp * vonkarman_unit_tab(u, tab_f) * m;
                        const double g = p.amp * vonkarman_slope_tab(u, tab_w) * m;
                        acc[1] -= 0.5 * g * dx * dx;
                        acc[2] -= g * dx * dy;
                        acc[3] -= 0.5 * g * dy * dy;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = acc[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < 4) out[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// Fixed-order sum of the workgroups' partial sums by one workgroup (the result does not depend on the schedule): nrb row blocks
// x nP panels, that order, of a partial array with `stride` panels per row block; the four sums to out[0 .. 3]
__device__ __forceinline__ void loglik_grad_reduce(const double *__restrict__ partial, int64_t nrb, int64_t nP, int64_t stride,
                                                   double *__restrict__ out) {
    __shared__ double red[256][4];
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q = tid; q < nrb * nP; q += 256) {
        const int64_t rb = q / nP, p = q % nP;
        for (int s = 0; s < 4; ++s) acc[s] += partial[(rb * stride + p) * 4 + s];
    }
    for (int s = 0; s < 4; ++s) red[tid][s] = acc[s];
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step)
            for (int s = 0; s < 4; ++s) red[tid][s] += red[tid + step][s];
        __syncthreads();
    }
    if (tid < 4) out[tid] = red[0][tid];
}
