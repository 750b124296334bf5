// Many small GPs in one launch sequence (seam S2e of include/tgp.h; replaces the reference's one cholesky + cho_solve per
// GP, treegp/gp_interp.py:180-182, and per likelihood evaluation, treegp/log_likelihood.py:29-33, 43-62).
//
// Every problem of a chunk is stored like a single solve at the chunk's common Np (packed panels): problem b's
// panels at b * tgp_panel_elems(Np), its inverted diagonal blocks at b * Np * 128; rows >= n_b carry the identity.  Every
// launch covers all problems of the chunk, the problem index being the grid's y dimension, and runs the existing device
// bodies through thin wrappers that only offset pointers by it:
//   K build        kbuild_tile (kbuild_tile.h), once per kernel evaluator present; problems whose kernel is a sum of two or more
//                  terms (seam S2i) through kbuild_tile_sum (ksum_eval.h), once per launch list present
//   posterior, gradient   the bodies of post_tile.h, which the single-problem kernels of cov.hip call too
//   per panel k    potrf128_body (0,0) -> rows below: X = A W0^T -> A[:,128:] -= X L10^T -> potrf128_body (1,1) ->
//                  rows below: X = A W1^T (gemm_tile_128) -> trailing update, depth 256 (gemm_tile_dtv)
//   sweeps         one launch per 128-block and direction: the block's GEMV with W = L_jj^-1 and the update of the other blocks
//   logdet, chi2   one workgroup per problem
// Plain launches on the context's one stream, no in-kernel waits, no atomics in any sum.  Tile forms and summation depths
// depend only on the panel index and Np, so a problem's bits do not depend on its companions, its place or the chunking.
// The posterior (S3f) and the likelihood gradient (S2f) of every problem follow from its factor in the same chunk, further down.
#define TGP_POTRF_BODY_ONLY
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "kbuild_tile.h"
#include "ksum_eval.h"
#include "gemm_tile.h"
#include "post_tile.h"
#include "potrf128.h"

namespace {

struct BatchDims {
    int64_t Np;
    int64_t ae;    // doubles per problem: packed panels
    int64_t we;    // doubles per problem: inverted diagonal blocks (Np x 128)
};

// ---- staging: the caller's (nb, nmax) rows -> (nb, Np) padded with zeros beyond n_b ---------------------------------------
__global__ __launch_bounds__(256) void bpad_kernel(const double *__restrict__ rX, const double *__restrict__ ry,
                                                   const double *__restrict__ re, const int64_t *__restrict__ ns, int64_t nmax,
                                                   int64_t Np, double *__restrict__ X, double *__restrict__ y, double *__restrict__ e) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Np) return;
    const bool in = i < ns[b];
    const int64_t s = (int64_t)b * nmax + i, d = (int64_t)b * Np + i;
    X[2 * d] = in ? rX[2 * s] : 0.0;
    X[2 * d + 1] = in ? rX[2 * s + 1] : 0.0;
    if (ry) y[d] = in ? ry[s] : 0.0;                            // (the K build alone stages no values)
    if (e) e[d] = in ? re[s] : 0.0;
}

// (nb, Np) -> the caller's (nb, nmax), exactly 0 beyond n_b
__global__ __launch_bounds__(256) void bunpad_kernel(const double *__restrict__ a, const int64_t *__restrict__ ns, int64_t nmax,
                                                     int64_t Np, double *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nmax) return;
    out[(int64_t)b * nmax + i] = i < ns[b] ? a[(int64_t)b * Np + i] : 0.0;
}

// ---- K + diag(yerr^2): one 128 x 128 tile per workgroup, blockIdx.y = the y-th problem of this launch list ---------------------
// Every problem's kernel is a KSumParams (ksum_eval.h); a one-term problem is its term 0 and goes through the evaluator's own
// launch, the problems of two or more terms through bkbuild_sum_kernel below.
template <int KE>
__global__ __launch_bounds__(256) void bkbuild_kernel(const KSumParams *__restrict__ ksp, const int *__restrict__ list,
                                                      const int64_t *__restrict__ ns, const double *__restrict__ X,
                                                      const double *__restrict__ e, BatchDims d, double *__restrict__ A) {
    const int b = list[blockIdx.y];
    int64_t ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int64_t pj = tj >> 1;
    double *tile = A + b * d.ae + panel_off(pj, d.Np) + (ti * TGP_TB - pj * TGP_PW) * TGP_PW + (tj & 1) * TGP_TB;
    const KParams p = ksp[b].t[0];
    kbuild_tile<KE>(p, X + (int64_t)b * 2 * d.Np, ns[b], e ? e + (int64_t)b * d.Np : nullptr, ti, tj, tile);
}

// The same tile for the problems of 2 .. TGP_SUM_MAX terms (seam S2i): every term in registers, the tile stored once
// (kbuild_tile_sum).  Two launch lists and two instantiations: ANYVK = false takes the sums of Gaussian terms only and carries no
// Bessel evaluator, ANYVK = true the sums with a von Karman term.  A problem's list follows from its own kernel alone.
template <bool ANYVK>
__global__ __launch_bounds__(256) void bkbuild_sum_kernel(const KSumParams *__restrict__ ksp, const int *__restrict__ list,
                                                          const int64_t *__restrict__ ns, const double *__restrict__ X,
                                                          const double *__restrict__ e, BatchDims d, double *__restrict__ A) {
    const int b = list[blockIdx.y];
    int64_t ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int64_t pj = tj >> 1;
    double *tile = A + b * d.ae + panel_off(pj, d.Np) + (ti * TGP_TB - pj * TGP_PW) * TGP_PW + (tj & 1) * TGP_TB;
    kbuild_tile_sum<ANYVK>(ksp[b], X + (int64_t)b * 2 * d.Np, ns[b], e ? e + (int64_t)b * d.Np : nullptr, ti, tj, tile);
}

// problem b's lower triangle with its diagonal from the packed panels to the caller's row-major (nmax x nmax) slot, exactly 0
// above the diagonal and beyond n_b; blockIdx.x = 256-column group + groups * row
__global__ __launch_bounds__(256) void bunpack_lower_kernel(const double *__restrict__ A, const int64_t *__restrict__ ns, BatchDims d,
                                                            int64_t nmax, double *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t ng = (nmax + 255) / 256;
    const int64_t i = blockIdx.x / ng;
    const int64_t j = (blockIdx.x % ng) * 256 + threadIdx.x;
    if (j >= nmax) return;
    const int64_t pj = j >> 8;
    out[((int64_t)b * nmax + i) * nmax + j] =
        (i < ns[b] && j <= i) ? A[b * d.ae + panel_off(pj, d.Np) + (i - pj * TGP_PW) * TGP_PW + (j & 255)] : 0.0;
}

// ---- factorisation ----------------------------------------------------------------------------------------------------------
// diagonal block at element `off` of every problem's panels, its inverse to element `woff` of its W; one workgroup each
__global__ __launch_bounds__(256) void bpotrf_kernel(double *A, double *W, BatchDims d, int64_t off, int64_t woff, int *info, int base) {
    const int b = blockIdx.x;
    potrf_v2::potrf128_body<true>(potrf_v2::potrf_lds_image, A + b * d.ae + off, TGP_PW, W + b * d.we + woff, info + b, base);
}

// a column of 128-row tiles of every problem: tile t uses A rows [128 t, +128) at element `ao`, the fixed B block at `bo` (of
// the panels, or of W when BW), C rows [128 t, +128) at `co`
template <int MODE, int LDB, bool BW>
__global__ __launch_bounds__(256, 2) void bgemm_col_kernel(double *A, const double *W, BatchDims d, int64_t ao, int64_t bo, int64_t co) {
    const int64_t t = blockIdx.x;
    double *Ab = A + blockIdx.y * d.ae;
    const double *B = BW ? W + blockIdx.y * d.we + bo : Ab + bo;
    gemm_tile_128<MODE, LDB, TGP_TB>(Ab + ao + t * TGP_TB * TGP_PW, B, Ab + co + t * TGP_TB * TGP_PW);
}

// trailing update after panel k: C(ti, tj) -= P[ti] P[tj]^T over the T x T lower tiles from block k + 1, depth 256
__global__ __launch_bounds__(256, 2) void bsyrk_kernel(double *A, BatchDims d, int k, int T) {
    int64_t ti, tj;
    tri_index(blockIdx.x, ti, tj);
    double *Ab = A + blockIdx.y * d.ae;
    const double *P = Ab + panel_off(k, d.Np) + (int64_t)TGP_PW * TGP_PW;      // panel k from row 256 (k + 1)
    const int ob = k + 1;
    const int64_t pj = ob + (tj >> 1);
    const int64_t I = (int64_t)TGP_PW * ob + TGP_TB * ti;
    double *C = Ab + panel_off(pj, d.Np) + (I - pj * TGP_PW) * TGP_PW + (tj & 1) * TGP_TB;
    gemm_tile_dtv<4, TGP_PW, 1>(P + ti * TGP_TB * TGP_PW, P + tj * TGP_TB * TGP_PW, C, nullptr, nullptr);
}

// ---- sweeps: GEMV pieces on 128-blocks --------------------------------------------------------------------------------------
// out[r] = sum_c M[r][c] v[c] for the 128 rows of M (ld `ldm`); wave w takes rows 32 w .. 32 w + 31, a row is one 1 KiB load of
// the wave and a butterfly over its lanes (the same tree for every row)
__device__ __forceinline__ void rows_dot128(const double *__restrict__ M, int ldm, const double *v, double *out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double v0 = v[2 * lane], v1 = v[2 * lane + 1];
    for (int r = 32 * w; r < 32 * w + 32; ++r) {
        const double2 m = *reinterpret_cast<const double2 *>(M + (int64_t)r * ldm + 2 * lane);
        double s = fma(m.y, v1, m.x * v0);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) out[r] = s;
    }
}
// out[c] = sum_r M[r][c] v[r]; thread (w, lane) sums columns 2 lane, 2 lane + 1 over rows 32 w .. 32 w + 31 in order, the four
// partial sums are then added in the order of w.  `part`: 4 x 128 doubles of LDS.  Ends with a barrier.
__device__ __forceinline__ void cols_dot128(const double *__restrict__ M, int ldm, const double *v, double *part, double *out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double2 s = {0.0, 0.0};
    for (int r = 32 * w; r < 32 * w + 32; ++r) {
        const double2 m = *reinterpret_cast<const double2 *>(M + (int64_t)r * ldm + 2 * lane);
        s.x = fma(m.x, v[r], s.x);
        s.y = fma(m.y, v[r], s.y);
    }
    part[w * 128 + 2 * lane] = s.x;
    part[w * 128 + 2 * lane + 1] = s.y;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c = threadIdx.x;
        out[c] = ((part[c] + part[128 + c]) + part[256 + c]) + part[384 + c];
    }
    __syncthreads();
}

// forward step j: every workgroup forms z_j = W_j y_j; workgroup 0 stores it, workgroup t >= 1 takes y_{j+t} -= L_{j+t,j} z_j
__global__ __launch_bounds__(256) void bfwd_step_kernel(const double *__restrict__ A, const double *__restrict__ W, BatchDims d,
                                                        double *y, double *z, int j) {
    __shared__ double v[128], zj[128], dv[128];
    const int b = blockIdx.y, t = blockIdx.x;
    y += b * d.Np;
    z += b * d.Np;
    if (threadIdx.x < 128) v[threadIdx.x] = y[(int64_t)j * TGP_TB + threadIdx.x];
    __syncthreads();
    rows_dot128(W + b * d.we + (int64_t)j * TGP_TB * TGP_TB, TGP_TB, v, zj);
    __syncthreads();
    if (t == 0) {
        if (threadIdx.x < 128) z[(int64_t)j * TGP_TB + threadIdx.x] = zj[threadIdx.x];
        return;
    }
    const int64_t i = j + t, pj = j >> 1;
    const double *L = A + b * d.ae + panel_off(pj, d.Np) + (i * TGP_TB - pj * TGP_PW) * TGP_PW + (j & 1) * TGP_TB;
    rows_dot128(L, TGP_PW, zj, dv);
    __syncthreads();
    if (threadIdx.x < 128) y[i * TGP_TB + threadIdx.x] -= dv[threadIdx.x];
}

// backward step j (descending): every workgroup forms a_j = W_j^T s_j; workgroup 0 stores it, workgroup t >= 1 takes
// s_{j-t} -= L_{j,j-t}^T a_j
__global__ __launch_bounds__(256) void bbwd_step_kernel(const double *__restrict__ A, const double *__restrict__ W, BatchDims d,
                                                        double *s, double *a, int j) {
    __shared__ double v[128], aj[128], dv[128], part[4 * 128];
    const int b = blockIdx.y, t = blockIdx.x;
    s += b * d.Np;
    a += b * d.Np;
    if (threadIdx.x < 128) v[threadIdx.x] = s[(int64_t)j * TGP_TB + threadIdx.x];
    __syncthreads();
    cols_dot128(W + b * d.we + (int64_t)j * TGP_TB * TGP_TB, TGP_TB, v, part, aj);
    if (t == 0) {
        if (threadIdx.x < 128) a[(int64_t)j * TGP_TB + threadIdx.x] = aj[threadIdx.x];
        return;
    }
    const int64_t i = j - t, pi = i >> 1;
    const double *L = A + b * d.ae + panel_off(pi, d.Np) + ((int64_t)j * TGP_TB - pi * TGP_PW) * TGP_PW + (i & 1) * TGP_TB;
    cols_dot128(L, TGP_PW, aj, part, dv);
    if (threadIdx.x < 128) s[i * TGP_TB + threadIdx.x] -= dv[threadIdx.x];
}

// logdet = sum 2 log L_ii and chi2 = |z|^2 over i < n_b: thread t sums i = t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void bfinish_kernel(const double *__restrict__ A, const double *__restrict__ z, const int64_t *__restrict__ ns,
                                                      BatchDims d, double *__restrict__ out) {
    __shared__ double sl[256], sz[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *Ab = A + b * d.ae, *zb = z + b * d.Np;
    const int64_t n = ns[b];
    double l = 0.0, q = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        const int64_t p = i / TGP_PW;
        l += 2.0 * log(Ab[panel_off(p, d.Np) + (i - p * TGP_PW) * TGP_PW + (i % TGP_PW)]);
        q = fma(zb[i], zb[i], q);
    }
    sl[tid] = l;
    sz[tid] = q;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            sl[tid] += sl[tid + h];
            sz[tid] += sz[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[2 * b] = sl[0];
        out[2 * b + 1] = sz[0];
    }
}

// ---- posterior of every problem (seam S3f): S3b / S3c of cov.hip with the problem index on the grid (post_tile.h) -----------
// Problem b's query rows live in the 256-wide panel layout of cov.hip's Bt: Bt_b (Mp x Np) at b * Mp * Np, panel p at
// + p * Mp * 256; the covariance's C_b (Mp x Mp) at b * Mp * Mp in the same layout.  Tile forms and summation depths depend on
// kb, Np and Mp only.  Row tiles at or beyond m_b and column blocks at or beyond n_b are zero from the start and stay zero, so a
// problem skips them: its own sizes decide which, never its companions'.
struct PostDims {
    int64_t Mp;
    int64_t mmax;
};

// H_b = amp_b k_b(Xs_b, X_b) (self: k_b(Xs_b, Xs_b), diagonal exactly amp_b): rows < m_b, columns < ncols_b, zero elsewhere.
// Every element of the Mp x ncols panels is written.  blockIdx.x = 256-column group + (ncols / 256) * row, blockIdx.y = the
// y-th problem of this evaluator.  Xs: the caller's (nb, mmax, 2) rows, read below m_b only; X: the staged (nb, Np, 2).
template <int KE>
__global__ __launch_bounds__(256) void bcross_kernel(const KSumParams *__restrict__ ksp, const int *__restrict__ list,
                                                     const int64_t *__restrict__ ns, const int64_t *__restrict__ ms,
                                                     const double *__restrict__ Xs, const double *__restrict__ X, int64_t Np,
                                                     PostDims q, int self, int64_t ncols, double *__restrict__ out) {
    const int b = list[blockIdx.y];
    const int64_t ng = ncols / 256;
    const int64_t i = blockIdx.x / ng;
    const int64_t j = (blockIdx.x % ng) * 256 + threadIdx.x;
    const int64_t m = ms[b], n = self ? m : ns[b];
    const double *xs = Xs + (int64_t)b * 2 * q.mmax;
    const double *x = self ? xs : X + (int64_t)b * 2 * Np;
    const KParams p = ksp[b].t[0];
    out[(int64_t)b * q.Mp * ncols + panel_elem(i, j, q.Mp)] = cross_value<KE>(p, xs, m, x, n, self, i, j);
}

// the same for the problems of 2 .. TGP_SUM_MAX terms: cross_value<KE> per term, added in term order (cross_value_sum); on
// `self` the diagonal is exactly the sum of the amplitudes.  Launch lists and instantiations as bkbuild_sum_kernel.
template <bool ANYVK>
__global__ __launch_bounds__(256) void bcross_sum_kernel(const KSumParams *__restrict__ ksp, const int *__restrict__ list,
                                                         const int64_t *__restrict__ ns, const int64_t *__restrict__ ms,
                                                         const double *__restrict__ Xs, const double *__restrict__ X, int64_t Np,
                                                         PostDims q, int self, int64_t ncols, double *__restrict__ out) {
    const int b = list[blockIdx.y];
    const int64_t ng = ncols / 256;
    const int64_t i = blockIdx.x / ng;
    const int64_t j = (blockIdx.x % ng) * 256 + threadIdx.x;
    const int64_t m = ms[b], n = self ? m : ns[b];
    const double *xs = Xs + (int64_t)b * 2 * q.mmax;
    const double *x = self ? xs : X + (int64_t)b * 2 * Np;
    out[(int64_t)b * q.Mp * ncols + panel_elem(i, j, q.Mp)] = cross_value_sum<ANYVK>(ksp[b], xs, m, x, n, self, i, j);
}

// Bt_b[:, kb] <- Bt_b[:, kb] W_kb^T, one 128-row tile per workgroup
__global__ __launch_bounds__(256, 2) void btrsm_kernel(double *Bt, const double *W, const int64_t *__restrict__ ns,
                                                       const int64_t *__restrict__ ms, BatchDims d, PostDims q, int kb) {
    const int b = blockIdx.y;
    const int64_t t = blockIdx.x;
    if (t * TGP_TB >= ms[b] || (int64_t)kb * TGP_TB >= ns[b]) return;
    double *Bk = Bt + (int64_t)b * q.Mp * d.Np + (int64_t)(kb >> 1) * q.Mp * TGP_PW + (kb & 1) * TGP_TB + t * TGP_TB * TGP_PW;
    post_trsm_tile(Bk, W + b * d.we + (int64_t)kb * TGP_TB * TGP_TB);
}

// Bt_b[:, c] -= Bt_b[:, kb] L_b[c, kb]^T for c = kb + 1 + blockIdx.x / mt, row tile blockIdx.x % mt
__global__ __launch_bounds__(256, 2) void bupdate_kernel(double *Bt, const double *A, const int64_t *__restrict__ ns,
                                                         const int64_t *__restrict__ ms, BatchDims d, PostDims q, int kb, int mt) {
    const int b = blockIdx.y;
    const int64_t ti = blockIdx.x % mt;
    const int64_t c = kb + 1 + blockIdx.x / mt;
    if (ti * TGP_TB >= ms[b] || c * TGP_TB >= ns[b]) return;
    post_update_tile(Bt + (int64_t)b * q.Mp * d.Np, q.Mp, A + b * d.ae, d.Np, kb, 0, ti, c);
}

// var_b[i] = amp_b - |Bt_b[i, :]|^2 over all Np / 256 panels, one wave per row (row_sqnorm_wave); rows >= m_b are 0.  amp_b: the
// prior variance, the amplitudes of problem b's terms added in term order
__global__ __launch_bounds__(256) void bvar_rows_kernel(const double *__restrict__ Bt, const KSumParams *__restrict__ ksp,
                                                        const int64_t *__restrict__ ms, int64_t Np, PostDims q,
                                                        double *__restrict__ var) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= q.mmax) return;                                     // whole waves leave together
    double *out = var + (int64_t)b * q.mmax + i;
    if (i >= ms[b]) {
        if (lane == 0) *out = 0.0;
        return;
    }
    const double acc = row_sqnorm_wave(Bt + (int64_t)b * q.Mp * Np, q.Mp, (int)(Np / TGP_PW), i);
    if (lane == 0) *out = ksp[b].ampsum - acc;
}

// C_b(ti, tj) -= sum over all panels of Bt_b[ti] Bt_b[tj]^T; blockIdx.x = ti + mt * tj
__global__ __launch_bounds__(256, 2) void bsyrk_cov_kernel(double *C, const double *Bt, const int64_t *__restrict__ ms, int64_t Np,
                                                           PostDims q, int mt) {
    const int b = blockIdx.y;
    const int64_t ti = blockIdx.x % mt, tj = blockIdx.x / mt;
    if (ti * TGP_TB >= ms[b] || tj * TGP_TB >= ms[b]) return;
    post_syrk_tile(C + (int64_t)b * q.Mp * q.Mp, Bt + (int64_t)b * q.Mp * Np, q.Mp, (int)(Np / TGP_PW), ti, tj, 0);
}

// C_b (panels) -> the caller's (nb, mmax, mmax), exactly 0 outside m_b x m_b; blockIdx.x = 256-column group + groups * row
__global__ __launch_bounds__(256) void bunpad_cov_kernel(const double *__restrict__ C, const int64_t *__restrict__ ms, PostDims q,
                                                         double *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t ng = (q.mmax + 255) / 256;
    const int64_t i = blockIdx.x / ng;
    const int64_t j = (blockIdx.x % ng) * 256 + threadIdx.x;
    if (j >= q.mmax) return;
    const int64_t m = ms[b];
    out[((int64_t)b * q.mmax + i) * q.mmax + j] =
        (i < m && j < m) ? C[(int64_t)b * q.Mp * q.Mp + panel_elem(i, j, q.Mp)] : 0.0;
}

// ---- likelihood gradient of every problem (seam S2f): S2d of cov.hip with the problem index on the grid (post_tile.h) ----------
// Problem b's Bt_b = L_b^-T and C_b = -K_b^-1 are Np x Np in the 256-wide panel layout of cov.hip (Bt_b at b * Np * Np, panel p
// at + p * Np * 256).  Bt_b starts as the identity and is upper triangular: row tile ti is zero left of column block ti, so the
// substitution's step kb covers the row tiles ti <= kb only (btrsm_kernel / bupdate_kernel above with kb + 1 row tiles, ms = ns)
// and C_b is formed over the lower tile pairs, each summed from panel ti / 2 on.  Nothing left of that is ever read, so nothing
// there is initialised.  Row tiles at or beyond n_b are skipped by the problem's own n_b; column blocks beyond it hold exact
// zeros in the rows below n_b.  Tile forms and summation depths depend on the tile indices and Np only, and the trailing
// zeros of a larger Np add nothing: a problem's bits do not depend on its companions, its place, the chunking or nmax.
struct GradDims {
    int64_t nrb;   // 64-row blocks of Np
    int64_t nP;    // 256-column panels of Np
};

// Bt_b <- identity, C_b <- 0 where they are read: row tile ti = blockIdx.x / nP below n_b, panel p = blockIdx.x % nP of Bt_b from
// ti / 2 on, of C_b up to ti / 2
__global__ __launch_bounds__(256) void bgrad_init_kernel(double *__restrict__ Bt, double *__restrict__ C, const int64_t *__restrict__ ns,
                                                         int64_t Np, int nP) {
    const int b = blockIdx.y;
    const int64_t ti = blockIdx.x / nP, p = blockIdx.x % nP;
    if (ti * TGP_TB >= ns[b]) return;
    const int64_t base = (int64_t)b * Np * Np + p * Np * TGP_PW + ti * TGP_TB * TGP_PW;
    const int r0 = threadIdx.x >> 7, c = 2 * (threadIdx.x & 127);
    if (p >= (ti >> 1)) {
        for (int r = r0; r < TGP_TB; r += 2) {
            const int64_t i = ti * TGP_TB + r, j = p * TGP_PW + c;
            double2 v = {j == i ? 1.0 : 0.0, j + 1 == i ? 1.0 : 0.0};
            *reinterpret_cast<double2 *>(Bt + base + (int64_t)r * TGP_PW + c) = v;
        }
    }
    if (p <= (ti >> 1)) {
        const double2 z = {0.0, 0.0};
        for (int r = r0; r < TGP_TB; r += 2) *reinterpret_cast<double2 *>(C + base + (int64_t)r * TGP_PW + c) = z;
    }
}

// lower tile pairs (ti >= tj), linear in blockIdx.x: C_b(ti, tj) = -sum_{p >= ti / 2} Bt_b[ti][p] Bt_b[tj][p]^T
__global__ __launch_bounds__(256, 2) void bkinv_syrk_kernel(double *C, const double *Bt, const int64_t *__restrict__ ns, int64_t Np, int nP) {
    const int b = blockIdx.y;
    int64_t ti, tj;
    tri_index(blockIdx.x, ti, tj);
    if (ti * TGP_TB >= ns[b]) return;
    post_syrk_tile(C + (int64_t)b * Np * Np, Bt + (int64_t)b * Np * Np, Np, nP, ti, tj, ti >> 1);
}

// loglik_grad_block<KE> for term `term` of problem b = list[blockIdx.y] (the chunk's problems whose term `term` has evaluator KE):
// 64 rows (blockIdx.x / nP) x one 256-column panel (blockIdx.x % nP) of the lower triangle below n_b, four partial sums per
// workgroup at partial[((b * T + term) * nrb * nP + blockIdx.x) * 4], T the rows of the result per problem (1, or TGP_SUM_MAX).  One launch per evaluator present and not one kernel that branches on kp[b].kind:
// the three bodies in one kernel take the von Karman bodies' 166 VGPRs (3 waves per SIMD) for the Gaussian problems too, whose
// own body needs 60 (8 waves per SIMD).  A problem's workgroups and sums are the same whichever launch its companions are in.
template <int KE>
__global__ __launch_bounds__(256) void bloglik_grad_kernel(const KSumParams *__restrict__ ksp, const int *__restrict__ list, int term,
                                                           int T, const int64_t *__restrict__ ns, const double *__restrict__ X,
                                                           const double *__restrict__ alpha, const double *__restrict__ C, int64_t Np,
                                                           GradDims g, double *__restrict__ partial) {
    const int b = list[blockIdx.y];
    const int64_t n = ns[b];
    const int64_t pj = blockIdx.x % g.nP, i0 = (int64_t)(blockIdx.x / g.nP) * 64;
    if (i0 >= n || pj * TGP_PW >= n) return;                      // whole workgroups leave together; never summed
    const KParams p = ksp[b].t[term];
    loglik_grad_block<KE>(p, X + (int64_t)b * 2 * Np, alpha + (int64_t)b * Np, C + (int64_t)b * Np * Np, Np, n, pj, i0,
                          partial + ((((int64_t)b * T + term) * g.nrb * g.nP) + blockIdx.x) * 4);
}

// one workgroup per problem (blockIdx.x) and term (blockIdx.y): its partial sums (row blocks below n_b x panels below n_b, that
// order) in a fixed order that depends on n_b alone.  Rows at or beyond the problem's term count are left as they are (zeroed
// by the host before the launch).
__global__ __launch_bounds__(256) void bloglik_grad_reduce_kernel(const double *__restrict__ partial, const KSumParams *__restrict__ ksp,
                                                                  int T, const int64_t *__restrict__ ns, GradDims g,
                                                                  double *__restrict__ out) {
    const int b = blockIdx.x, t = blockIdx.y;
    if (t >= ksp[b].nterms) return;
    const int64_t n = ns[b];
    loglik_grad_reduce(partial + ((int64_t)b * T + t) * g.nrb * g.nP * 4, (n + 63) / 64, (n + TGP_PW - 1) / TGP_PW, g.nP,
                       out + ((int64_t)b * T + t) * 4);
}

// ---- diag(K^-1) of every problem (seam S2g): the substitution of S2f without its C_b ---------------------------------------------
// Bt_b = L_b^-T as above (Np x Np panels at b * Np * Np, the same init region, the same substitution launches); row i of it is
// L_b^-1 e_i, so [K_b^-1]_ii is its squared norm, taken from the row's own panel (i / 128) / 2 on: nothing left of the
// initialised region is read.  The panels behind n_b hold exact zeros in the rows below n_b and come last in the sum, so a larger
// Np changes no bit.

// Bt_b <- identity where the substitution reads it: row tile ti = blockIdx.x / nP below n_b, panel p = blockIdx.x % nP from ti / 2 on
__global__ __launch_bounds__(256) void binv_init_kernel(double *__restrict__ Bt, const int64_t *__restrict__ ns, int64_t Np, int nP) {
    const int b = blockIdx.y;
    const int64_t ti = blockIdx.x / nP, p = blockIdx.x % nP;
    if (ti * TGP_TB >= ns[b] || p < (ti >> 1)) return;
    const int64_t base = (int64_t)b * Np * Np + p * Np * TGP_PW + ti * TGP_TB * TGP_PW;
    const int r0 = threadIdx.x >> 7, c = 2 * (threadIdx.x & 127);
    for (int r = r0; r < TGP_TB; r += 2) {
        const int64_t i = ti * TGP_TB + r, j = p * TGP_PW + c;
        double2 v = {j == i ? 1.0 : 0.0, j + 1 == i ? 1.0 : 0.0};
        *reinterpret_cast<double2 *>(Bt + base + (int64_t)r * TGP_PW + c) = v;
    }
}

// invdiag_b[i] = |Bt_b[i, :]|^2 over the panels (i / 128) / 2 .. Np / 256 - 1, one wave per row (row_sqnorm_wave_from); rows
// >= n_b of the caller's (nb, nmax) layout are exactly 0
__global__ __launch_bounds__(256) void binv_diag_kernel(const double *__restrict__ Bt, const int64_t *__restrict__ ns, int64_t Np,
                                                        int64_t nmax, double *__restrict__ invdiag) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nmax) return;                                       // whole waves leave together
    double *out = invdiag + (int64_t)b * nmax + i;
    if (i >= ns[b]) {
        if (lane == 0) *out = 0.0;
        return;
    }
    const double acc = row_sqnorm_wave_from(Bt + (int64_t)b * Np * Np, Np, (int)(Np / TGP_PW), i, (int)((i / TGP_TB) >> 1));
    if (lane == 0) *out = acc;
}

}  // namespace

// problems per chunk: TGP_BATCH_CHUNK, or as many as 90 % of the free device memory holds (the context's own scratch counted as
// free: it is given back before a bigger one is taken)
static int64_t batch_chunk(tgp_ctx *ctx, const char *fn, int nb, size_t per, size_t fixed, int *rc) {
    *rc = 0;
    const char *e = getenv("TGP_BATCH_CHUNK");                // read per call, as TGP_VAR_CHUNK is
    if (e && atoi(e) > 0) {
        const int64_t c = atoi(e) < nb ? atoi(e) : nb;
        return c < 65535 ? c : 65535;
    }
    size_t fr = 0, tot = 0;
    hipError_t he = hipMemGetInfo(&fr, &tot);
    if (he != hipSuccess) {
        ctx->err = std::string("hipMemGetInfo: ") + hipGetErrorString(he);
        *rc = -2;
        return 0;
    }
    const double avail = 0.9 * (double)(fr + ctx->scratch_bytes) - (double)fixed;
    int64_t c = avail > 0 ? (int64_t)(avail / (double)per) : 0;
    if (c > nb) c = nb;
    if (c > 65535) c = 65535;                                   // the problem index is a grid's y dimension
    if (c < 1) {
        ctx->err = std::string(fn) + ": not enough free device memory for one problem of this order";
        *rc = -2;
    }
    return c;
}

// The kernels of a batch: the one kernel per problem of the entries of S2e .. S3f, or the sums of seam S2i.  The core below takes
// sums; an old entry's problems are sums of one term.
struct KSrc {
    const tgp_kernel *k1;
    const tgp_kernel_sum *ks;
    int nterms(int64_t b) const { return ks ? ks[b].nterms : 1; }
    const tgp_kernel *term(int64_t b, int t) const { return ks ? &ks[b].term[t] : &k1[b]; }
};

// nb, nmax, ns[b] and the kinds (of a sum: the term count and every term's kind), as every batched entry takes them; -1 with a
// message naming `fn`, the problem and the term
static int batch_check(tgp_ctx *ctx, const char *fn, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax) {
    const std::string f(fn);
    if (nb < 1) { ctx->err = f + ": nb must be >= 1"; return -1; }
    if (nmax < 1 || nmax > 4096) { ctx->err = f + ": nmax must be in 1 .. 4096 (larger problems: tgp_gp_solve)"; return -1; }
    for (int b = 0; b < nb; ++b) {
        if (ns[b] < 1 || ns[b] > nmax) {
            ctx->err = f + ": ns[" + std::to_string(b) + "] = " + std::to_string((long long)ns[b]) + " is not in 1 .. nmax = " +
                       std::to_string((long long)nmax);
            return -1;
        }
        if (!ks.ks) {
            if (kind_to_ke(ks.k1[b].kind) < 0) {
                ctx->err = f + ": ks[" + std::to_string(b) + "].kind = " + std::to_string(ks.k1[b].kind) + " is not a kernel kind";
                return -1;
            }
            continue;
        }
        const int nt = ks.ks[b].nterms;
        if (nt < 1 || nt > TGP_SUM_MAX) {
            ctx->err = f + ": ks[" + std::to_string(b) + "].nterms = " + std::to_string(nt) + " is outside 1 .. " +
                       std::to_string(TGP_SUM_MAX);
            return -1;
        }
        for (int t = 0; t < nt; ++t)
            if (kind_to_ke(ks.ks[b].term[t].kind) < 0) {
                ctx->err = f + ": ks[" + std::to_string(b) + "].term[" + std::to_string(t) + "].kind = " +
                           std::to_string(ks.ks[b].term[t].kind) + " is not a kernel kind";
                return -1;
            }
    }
    return 0;
}

// launch lists of the kernels that evaluate kernel values (K build, cross panels): the one-term problems by evaluator, then the
// sums of Gaussian terms only, then the sums with a von Karman term
enum { BL_GAUSS = 0, BL_VK = 1, BL_AVK = 2, BL_SUM_GAUSS = 3, BL_SUM_VK = 4, BL_N = 5 };

// the per-problem arrays of one chunk of S2e (device arena + pinned host tables); the posterior's own arrays follow them
struct BatchBufs {
    double *dA, *dW, *dX, *dy, *de, *dz, *da, *rX, *ry, *re, *ra, *dout;
    KSumParams *dks;
    int64_t *dns;
    int *dlist, *dglist, *dinfo;
    KSumParams *hks;
    int64_t *hns;
    int *hlist, *hglist, *hinfo;
    double *hout;
    int cnt[BL_N], start[BL_N];    // the chunk's launch lists: problems per list and where each starts in dlist
};

static size_t batch_bytes_per_problem(const BatchDims &d, int64_t nmax) {
    return rup((size_t)d.ae * 8) + rup((size_t)d.we * 8) + 6 * rup((size_t)d.Np * 8) + 5 * rup((size_t)nmax * 8) +
           rup(sizeof(KSumParams)) + 2 * rup(8) + 3 * rup(16);
}

// carves C problems' arrays of S2e out of the arena at `base` (+ *off) and the pinned host scratch
static int batch_take(tgp_ctx *ctx, const BatchDims &d, int64_t nmax, int64_t C, char *base, size_t *off, BatchBufs *bb) {
    auto take = [&](size_t bytes) { void *p = base + *off; *off += rup(bytes); return p; };
    const int64_t Np = d.Np;
    bb->dA = (double *)take((size_t)C * d.ae * 8);
    bb->dW = (double *)take((size_t)C * d.we * 8);
    bb->dX = (double *)take((size_t)C * 2 * Np * 8);
    bb->dy = (double *)take((size_t)C * Np * 8);
    bb->de = (double *)take((size_t)C * Np * 8);
    bb->dz = (double *)take((size_t)C * Np * 8);
    bb->da = (double *)take((size_t)C * Np * 8);
    bb->rX = (double *)take((size_t)C * 2 * nmax * 8);
    bb->ry = (double *)take((size_t)C * nmax * 8);
    bb->re = (double *)take((size_t)C * nmax * 8);
    bb->ra = (double *)take((size_t)C * nmax * 8);
    bb->dks = (KSumParams *)take((size_t)C * sizeof(KSumParams));
    bb->dns = (int64_t *)take((size_t)C * 8);
    bb->dlist = (int *)take((size_t)C * 4);
    bb->dglist = (int *)take((size_t)C * 4 * TGP_SUM_MAX);     // the gradient's lists: one set per term (solve_grad_batch)
    bb->dinfo = (int *)take((size_t)C * 4);
    bb->dout = (double *)take((size_t)C * 16);
    // host side of the small tables and results: the context's pinned scratch
    const size_t hbytes = rup((size_t)C * sizeof(KSumParams)) + rup((size_t)C * 8) + rup((size_t)C * 4) +
                          rup((size_t)C * 4 * TGP_SUM_MAX) + rup((size_t)C * 4) + rup((size_t)C * 16);
    void *hp = nullptr;
    int rc = tgp_ensure_pinned(ctx, hbytes, &hp);
    if (rc) return rc;
    char *hb = (char *)hp;
    bb->hks = (KSumParams *)hb;
    bb->hns = (int64_t *)(hb + rup((size_t)C * sizeof(KSumParams)));
    bb->hlist = (int *)((char *)bb->hns + rup((size_t)C * 8));
    bb->hglist = (int *)((char *)bb->hlist + rup((size_t)C * 4));
    bb->hinfo = (int *)((char *)bb->hglist + rup((size_t)C * 4 * TGP_SUM_MAX));
    bb->hout = (double *)((char *)bb->hinfo + rup((size_t)C * 4));
    static bool attr_ok = hipFuncSetAttribute((const void *)bpotrf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)potrf_v2::POTRF_LDS_BYTES) == hipSuccess;
    if (!attr_ok) { ctx->err = "batched solve: the diagonal-block kernel cannot have its LDS image"; return -2; }
    return 0;
}

// the launch list of problem b's kernel: decided by that kernel alone
static int batch_list_of(const KSumParams &k) {
    if (k.nterms == 1) return k.ke[0];                            // (BL_GAUSS .. BL_AVK are the evaluators' own numbers)
    return k.any_vk ? BL_SUM_VK : BL_SUM_GAUSS;
}

// problems c0 .. c0 + cn of the batch: the small tables and the caller's rows to the device, the rows padded to Np, then
// K + diag(yerr^2) of every problem into its packed panels (ev[0] .. ev[1]), one launch per launch list present.  y may be NULL.
static int batch_build_chunk(tgp_ctx *ctx, const BatchDims &d, BatchBufs &bb, int64_t c0, int64_t cn, const KSrc &ks,
                             const int64_t *ns, int64_t nmax, const double *X, const double *y, const double *yerr) {
    hipStream_t st = ctx->stream;
    const int64_t Np = d.Np, nT = Np / TGP_TB;
    // launch lists: the problems of this chunk grouped by what their kernel needs, each group in batch order
    int *cnt = bb.cnt, *start = bb.start;
    for (int l = 0; l < BL_N; ++l) cnt[l] = 0;
    for (int64_t b = 0; b < cn; ++b) {
        const int64_t gb = c0 + b;
        bb.hks[b] = make_ksum_terms(ks.nterms(gb), [&](int t) { return ks.term(gb, t); }, false);
        bb.hns[b] = ns[gb];
        ++cnt[batch_list_of(bb.hks[b])];
    }
    start[0] = 0;
    for (int l = 1; l < BL_N; ++l) start[l] = start[l - 1] + cnt[l - 1];
    int fill[BL_N] = {0, 0, 0, 0, 0};
    for (int64_t b = 0; b < cn; ++b) {
        const int l = batch_list_of(bb.hks[b]);
        bb.hlist[start[l] + fill[l]++] = (int)b;
    }
    TGP_HIP(hipMemcpyAsync(bb.dks, bb.hks, (size_t)cn * sizeof(KSumParams), hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(bb.dns, bb.hns, (size_t)cn * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(bb.dlist, bb.hlist, (size_t)cn * 4, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(bb.rX, X + c0 * nmax * 2, (size_t)cn * nmax * 16, hipMemcpyHostToDevice, st));
    if (y) TGP_HIP(hipMemcpyAsync(bb.ry, y + c0 * nmax, (size_t)cn * nmax * 8, hipMemcpyHostToDevice, st));
    if (yerr) TGP_HIP(hipMemcpyAsync(bb.re, yerr + c0 * nmax, (size_t)cn * nmax * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemsetAsync(bb.dinfo, 0, (size_t)cn * 4, st));
    const unsigned ncn = (unsigned)cn;
    double *dA = bb.dA;
    bpad_kernel<<<dim3((unsigned)(Np / 256), ncn), 256, 0, st>>>(bb.rX, y ? bb.ry : nullptr, yerr ? bb.re : nullptr, bb.dns, nmax, Np,
                                                                 bb.dX, bb.dy, yerr ? bb.de : nullptr);
    const double *e_or_null = yerr ? bb.de : nullptr;

    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    const unsigned ntiles = (unsigned)(nT * (nT + 1) / 2);
#define TGP_BUILD(KERNEL, l)                                                                                                      \
    if (cnt[l]) KERNEL<<<dim3(ntiles, cnt[l]), 256, 0, st>>>(bb.dks, bb.dlist + start[l], bb.dns, bb.dX, e_or_null, d, dA);
    TGP_BUILD(bkbuild_kernel<KE_GAUSS>, BL_GAUSS)
    TGP_BUILD(bkbuild_kernel<KE_VK>, BL_VK)
    TGP_BUILD(bkbuild_kernel<KE_AVK>, BL_AVK)
    TGP_BUILD(bkbuild_sum_kernel<false>, BL_SUM_GAUSS)
    TGP_BUILD(bkbuild_sum_kernel<true>, BL_SUM_VK)
#undef TGP_BUILD
    TGP_HIP(hipEventRecord(ctx->ev[1], st));
    TGP_HIP(hipGetLastError());
    return 0;
}

// problems c0 .. c0 + cn of the batch: staging and K build (batch_build_chunk), factorisation, sweeps and logdet / chi2, on the
// context's stream; alpha (padded, Np) in bb.da and unpadded in bb.ra when `want_alpha`.  Events: ev[0] .. ev[1] K build, .. ev[2]
// Cholesky, .. ev[3] sweeps.  Nothing is copied back and the stream is not synchronised.
static int batch_factor_chunk(tgp_ctx *ctx, const BatchDims &d, BatchBufs &bb, int64_t c0, int64_t cn, const KSrc &ks,
                              const int64_t *ns, int64_t nmax, const double *X, const double *y, const double *yerr, bool want_alpha) {
    int rc = batch_build_chunk(ctx, d, bb, c0, cn, ks, ns, nmax, X, y, yerr);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const int64_t Np = d.Np, nP = Np / TGP_PW, nT = Np / TGP_TB;
    const unsigned ncn = (unsigned)cn;
    double *dA = bb.dA, *dW = bb.dW;

    // right-looking, one 256-wide panel at a time
    for (int k = 0; k < (int)nP; ++k) {
        const int64_t pk = panel_off(k, Np), mk = Np - (int64_t)TGP_PW * k;
        const int64_t w0 = (int64_t)(2 * k) * TGP_TB * TGP_TB, w1 = w0 + TGP_TB * TGP_TB;
        const int64_t r1 = pk + (int64_t)TGP_TB * TGP_PW;          // row 128 of the panel
        const unsigned nr1 = (unsigned)((mk - TGP_TB) / TGP_TB), nr2 = (unsigned)((mk - TGP_PW) / TGP_TB);
        bpotrf_kernel<<<ncn, 256, potrf_v2::POTRF_LDS_BYTES, st>>>(dA, dW, d, pk, w0, bb.dinfo, k * TGP_PW);
        bgemm_col_kernel<0, TGP_TB, true><<<dim3(nr1, ncn), 256, 0, st>>>(dA, dW, d, r1, w0, r1);
        bgemm_col_kernel<1, TGP_PW, false><<<dim3(nr1, ncn), 256, 0, st>>>(dA, dW, d, r1, r1, r1 + TGP_TB);
        bpotrf_kernel<<<ncn, 256, potrf_v2::POTRF_LDS_BYTES, st>>>(dA, dW, d, r1 + TGP_TB, w1, bb.dinfo, k * TGP_PW + TGP_TB);
        if (nr2 == 0) continue;
        const int64_t r2 = pk + (int64_t)TGP_PW * TGP_PW + TGP_TB;   // row 256, column 128
        bgemm_col_kernel<0, TGP_TB, true><<<dim3(nr2, ncn), 256, 0, st>>>(dA, dW, d, r2, w1, r2);
        bsyrk_kernel<<<dim3((unsigned)(nr2 * (nr2 + 1) / 2), ncn), 256, 0, st>>>(dA, d, k, (int)nr2);
    }
    TGP_HIP(hipEventRecord(ctx->ev[2], st));

    for (int j = 0; j < (int)nT; ++j)
        bfwd_step_kernel<<<dim3((unsigned)(nT - j), ncn), 256, 0, st>>>(dA, dW, d, bb.dy, bb.dz, j);
    bfinish_kernel<<<ncn, 256, 0, st>>>(dA, bb.dz, bb.dns, d, bb.dout);
    if (want_alpha) {
        for (int j = (int)nT - 1; j >= 0; --j)
            bbwd_step_kernel<<<dim3((unsigned)(j + 1), ncn), 256, 0, st>>>(dA, dW, d, bb.dz, bb.da, j);
        bunpad_kernel<<<dim3((unsigned)((nmax + 255) / 256), ncn), 256, 0, st>>>(bb.da, bb.dns, nmax, Np, bb.ra);
    }
    TGP_HIP(hipEventRecord(ctx->ev[3], st));
    TGP_HIP(hipGetLastError());
    return 0;
}

// after the stream has been synchronised: the chunk's info, logdet and chi2 to the caller's arrays
static int batch_collect(tgp_ctx *ctx, const char *fn, const BatchBufs &bb, int64_t c0, int64_t cn, double *logdet, double *ydota,
                         int32_t *info) {
    for (int64_t b = 0; b < cn; ++b) {
        if (bb.hinfo[b] < 0) {
            ctx->err = std::string(fn) + ": a diagonal block of problem " + std::to_string((long long)(c0 + b)) +
                       " reported an internal hand-off failure (info " + std::to_string(bb.hinfo[b]) + ")";
            return -2;
        }
        info[c0 + b] = bb.hinfo[b];
        logdet[c0 + b] = bb.hout[2 * b];
        if (ydota) ydota[c0 + b] = bb.hout[2 * b + 1];
    }
    return 0;
}

// One batched call: the geometry, the caller's host arrays of S2e, the chunk size, the arena with S2e's arrays taken (the caller
// takes its own behind them with take()) and the phase times summed over the chunks.
struct BatchRun {
    tgp_ctx *ctx;
    const char *fn;
    int nb;
    int64_t nmax;
    double *alpha, *logdet, *ydota;
    int32_t *info;
    BatchDims d;
    int64_t C;          // problems per chunk
    char *base;
    size_t off;
    BatchBufs bb;
    double ms[5];       // K build, Cholesky, sweeps, the caller's device work (ev[4] .. ev[5]), its result's transfer (ev[5] .. ev[6])
    void *take(size_t bytes) { void *p = base + off; off += rup(bytes); return p; }
};

// after the caller's own NULL checks: nb, nmax, ns and the kinds (batch_check), then the geometry.  Touches no device.
static int batch_begin(BatchRun &r, tgp_ctx *ctx, const char *fn, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax,
                       double *alpha, double *logdet, double *ydota, int32_t *info) {
    int rc = batch_check(ctx, fn, nb, ks, ns, nmax);
    if (rc) return rc;
    const int64_t Np = padded_n(nmax);
    r = BatchRun{ctx, fn, nb, nmax, alpha, logdet, ydota, info, {Np, panel_off(Np / TGP_PW, Np), Np * TGP_TB}};
    return 0;
}

// the chunk size for S2e's bytes per problem plus the caller's `extra`, one arena per chunk size (arrays of C problems each),
// S2e's arrays taken from it
static int batch_arena(BatchRun &r, size_t extra) {
    tgp_ctx *ctx = r.ctx;
    TGP_HIP(hipSetDevice(ctx->device));
    const size_t per = batch_bytes_per_problem(r.d, r.nmax) + extra;
    const size_t fixed = 8 * 256;
    int rc = 0;
    r.C = batch_chunk(ctx, r.fn, r.nb, per, fixed, &rc);
    if (rc) return rc;
    rc = tgp_ensure_scratch(ctx, (size_t)r.C * per + fixed);
    if (rc) return rc;
    r.base = (char *)ctx->scratch;
    r.off = 0;
    return batch_take(ctx, r.d, r.nmax, r.C, r.base, &r.off, &r.bb);
}

// End of chunk c0 .. c0 + cn: info, logdet / chi2, alpha (when asked for) and the caller's result (`res`, or NULL) to the host, in
// that order; next = 2 records ev[6] behind them.  Synchronises the stream, adds the chunk's phase times (ev[0] .. ev[3] and the
// caller's `next` intervals from ev[4] on) and hands info, logdet and chi2 to the caller's arrays.
static int batch_end_chunk(BatchRun &r, int64_t c0, int64_t cn, void *res, const void *dres, size_t res_bytes, int next) {
    tgp_ctx *ctx = r.ctx;
    hipStream_t st = ctx->stream;
    const BatchBufs &bb = r.bb;
    TGP_HIP(hipMemcpyAsync(bb.hinfo, bb.dinfo, (size_t)cn * 4, hipMemcpyDeviceToHost, st));
    TGP_HIP(hipMemcpyAsync(bb.hout, bb.dout, (size_t)cn * 16, hipMemcpyDeviceToHost, st));
    if (r.alpha) TGP_HIP(hipMemcpyAsync(r.alpha + c0 * r.nmax, bb.ra, (size_t)cn * r.nmax * 8, hipMemcpyDeviceToHost, st));
    if (res) TGP_HIP(hipMemcpyAsync(res, dres, res_bytes, hipMemcpyDeviceToHost, st));
    if (next == 2) TGP_HIP(hipEventRecord(ctx->ev[6], st));
    TGP_HIP(hipStreamSynchronize(st));
    static const int from[5] = {0, 1, 2, 4, 5};
    for (int i = 0; i < 3 + next; ++i) {
        float t = 0.f;
        TGP_HIP(hipEventElapsedTime(&t, ctx->ev[from[i]], ctx->ev[from[i] + 1]));
        r.ms[i] += t;
    }
    return batch_collect(ctx, r.fn, bb, c0, cn, r.logdet, r.ydota, r.info);
}

// only the slots a batched call fills: nothing of an earlier call on the context is left behind in the others
static void batch_finish(const BatchRun &r) {
    static const int slot[5] = {0, 1, 2, 3, 9};
    for (int i = 0; i < TGP_NTIMINGS; ++i) r.ctx->timings[i] = 0.0;
    for (int i = 0; i < 5; ++i) r.ctx->timings[slot[i]] = r.ms[i];
}

static int solve_batch(tgp_ctx *ctx, const char *fn, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax, const double *X,
                       const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info) {
    if (!ctx) return -1;
    TGP_ARG((ks.k1 || ks.ks) && ns && X && y && logdet && info);
    BatchRun r;
    int rc = batch_begin(r, ctx, fn, nb, ks, ns, nmax, alpha, logdet, ydota, info);
    if (rc) return rc;
    rc = batch_arena(r, 0);
    if (rc) return rc;
    for (int64_t c0 = 0; c0 < nb; c0 += r.C) {
        const int64_t cn = (nb - c0) < r.C ? (nb - c0) : r.C;
        rc = batch_factor_chunk(ctx, r.d, r.bb, c0, cn, ks, ns, nmax, X, y, yerr, alpha != nullptr);
        if (rc) return rc;
        rc = batch_end_chunk(r, c0, cn, nullptr, nullptr, 0, 0);
        if (rc) return rc;
    }
    batch_finish(r);
    ctx->timings[10] = alpha ? 2.0 : 1.0;
    return 0;
}

int tgp_gp_solve_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                       const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info) {
    return solve_batch(ctx, "tgp_gp_solve_batch", nb, KSrc{ks, nullptr}, ns, nmax, X, y, yerr, alpha, logdet, ydota, info);
}

int tgp_gp_solve_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                           const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info) {
    return solve_batch(ctx, "tgp_gp_solve_batch_sum", nb, KSrc{nullptr, ks}, ns, nmax, X, y, yerr, alpha, logdet, ydota, info);
}

// ---- S2i: the batched K build alone, every problem's lower triangle back on the host (the building block of seam S2i) --------
int tgp_kbuild_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                         const double *yerr, double *K) {
    static const char *fn = "tgp_kbuild_batch_sum";
    if (!ctx) return -1;
    if (!(ks && ns && X && K)) {
        ctx->err = "tgp_kbuild_batch_sum: ks, ns, X and K must not be NULL";
        return -1;
    }
    BatchRun r;
    int rc = batch_begin(r, ctx, fn, nb, KSrc{nullptr, ks}, ns, nmax, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    // per problem beside S2e's arrays: the lower triangle in the caller's layout
    rc = batch_arena(r, rup((size_t)nmax * nmax * 8));
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const int64_t C = r.C;
    double *dK = (double *)r.take((size_t)C * nmax * nmax * 8);
    double ms = 0.0;
    for (int64_t c0 = 0; c0 < nb; c0 += C) {
        const int64_t cn = (nb - c0) < C ? (nb - c0) : C;
        rc = batch_build_chunk(ctx, r.d, r.bb, c0, cn, KSrc{nullptr, ks}, ns, nmax, X, nullptr, yerr);
        if (rc) return rc;
        bunpack_lower_kernel<<<dim3((unsigned)(nmax * ((nmax + 255) / 256)), (unsigned)cn), 256, 0, st>>>(r.bb.dA, r.bb.dns, r.d, nmax, dK);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipMemcpyAsync(K + (size_t)c0 * nmax * nmax, dK, (size_t)cn * nmax * nmax * 8, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipStreamSynchronize(st));
        float t = 0.f;
        TGP_HIP(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
        ms += t;
    }
    for (int i = 0; i < TGP_NTIMINGS; ++i) ctx->timings[i] = 0.0;
    ctx->timings[0] = ms;
    return 0;
}

// ---- S3f: the posterior variance or covariance of every problem of S2e from its factor, in the same call -------------------
// Per chunk, after batch_factor_chunk: H_b into Bt_b (and Kss_b into C_b), the block substitution Bt_b <- H_b L_b^-T over the
// 128-column blocks kb (trsm with W_kb, update of the blocks to its right), then amp_b - |Bt_b[i, :]|^2 or Kss_b - Bt_b Bt_b^T,
// unpadded to the caller's layout on the device.
#define TGP_POST_VAR_MMAX TGP_VAR_CHUNK_MAX       // the variance's rows go through a row grid, as in cov.hip
#define TGP_POST_COV_MMAX 4096

static int posterior_batch(tgp_ctx *ctx, const char *fn, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax, const double *X,
                           const double *y, const double *yerr, const int64_t *ms, int64_t mmax, const double *Xs, int what,
                           double *alpha, double *unc, double *logdet, double *ydota, int32_t *info) {
    if (!ctx) return -1;
    if (!((ks.k1 || ks.ks) && ns && X && y && ms && Xs && unc && logdet && info)) {
        ctx->err = std::string(fn) + ": ks, ns, X, y, ms, Xs, unc, logdet and info must not be NULL";
        return -1;
    }
    if (what != 1 && what != 2) {
        ctx->err = std::string(fn) + ": what = " + std::to_string(what) + " is neither 1 (variance) nor 2 (covariance)";
        return -1;
    }
    BatchRun r;
    int rc = batch_begin(r, ctx, fn, nb, ks, ns, nmax, alpha, logdet, ydota, info);
    if (rc) return rc;
    const bool cov = what == 2;
    const int64_t mlim = cov ? TGP_POST_COV_MMAX : TGP_POST_VAR_MMAX;
    if (mmax < 1 || mmax > mlim) {
        ctx->err = std::string(fn) + ": mmax must be in 1 .. " + std::to_string((long long)mlim) + (cov ? " for the covariance" : " for the variance");
        return -1;
    }
    for (int b = 0; b < nb; ++b)
        if (ms[b] < 1 || ms[b] > mmax) {
            ctx->err = std::string(fn) + ": ms[" + std::to_string(b) + "] = " + std::to_string((long long)ms[b]) + " is not in 1 .. mmax = " +
                       std::to_string((long long)mmax);
            return -1;
        }
    hipStream_t st = ctx->stream;
    const BatchDims &d = r.d;
    const int64_t Np = d.Np, nT = Np / TGP_TB;
    const PostDims q{(mmax + TGP_PW - 1) / TGP_PW * TGP_PW, mmax};
    const int mt = (int)(q.Mp / TGP_TB);
    // per problem beside S2e's arrays: Bt, the query rows, ms, the result on the device (panels for the covariance) and unpadded
    const size_t out_elems = cov ? (size_t)mmax * mmax : (size_t)mmax;
    rc = batch_arena(r, rup((size_t)q.Mp * Np * 8) + rup((size_t)mmax * 16) + rup(8) + (cov ? rup((size_t)q.Mp * q.Mp * 8) : 0) +
                            rup(out_elems * 8));
    if (rc) return rc;
    const int64_t C = r.C;
    BatchBufs &bb = r.bb;
    double *dBt = (double *)r.take((size_t)C * q.Mp * Np * 8);
    double *dXs = (double *)r.take((size_t)C * mmax * 16);
    int64_t *dms = (int64_t *)r.take((size_t)C * 8);
    double *dC = cov ? (double *)r.take((size_t)C * q.Mp * q.Mp * 8) : nullptr;
    double *dU = (double *)r.take((size_t)C * out_elems * 8);

    for (int64_t c0 = 0; c0 < nb; c0 += C) {
        const int64_t cn = (nb - c0) < C ? (nb - c0) : C;
        const unsigned ncn = (unsigned)cn;
        rc = batch_factor_chunk(ctx, d, bb, c0, cn, ks, ns, nmax, X, y, yerr, alpha != nullptr);
        if (rc) return rc;
        TGP_HIP(hipMemcpyAsync(dms, ms + c0, (size_t)cn * 8, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(dXs, Xs + c0 * mmax * 2, (size_t)cn * mmax * 16, hipMemcpyHostToDevice, st));
        TGP_HIP(hipEventRecord(ctx->ev[4], st));
        // H_b (and Kss_b), one launch per launch list present, as the K build
        const unsigned gh = (unsigned)(q.Mp * (Np / 256)), gk = (unsigned)(q.Mp * (q.Mp / 256));
        const int *cnt = bb.cnt, *start = bb.start;
#define TGP_CROSS(KERNEL, i)                                                                                                      \
        if (cnt[i]) {                                                                                                                 \
            KERNEL<<<dim3(gh, cnt[i]), 256, 0, st>>>(bb.dks, bb.dlist + start[i], bb.dns, dms, dXs, bb.dX, Np, q, 0, Np, dBt);      \
            if (cov) KERNEL<<<dim3(gk, cnt[i]), 256, 0, st>>>(bb.dks, bb.dlist + start[i], bb.dns, dms, dXs, bb.dX, Np, q, 1, q.Mp, dC); \
        }
        TGP_CROSS(bcross_kernel<KE_GAUSS>, BL_GAUSS)
        TGP_CROSS(bcross_kernel<KE_VK>, BL_VK)
        TGP_CROSS(bcross_kernel<KE_AVK>, BL_AVK)
        TGP_CROSS(bcross_sum_kernel<false>, BL_SUM_GAUSS)
        TGP_CROSS(bcross_sum_kernel<true>, BL_SUM_VK)
#undef TGP_CROSS
        // Bt_b <- H_b L_b^-T
        for (int kb = 0; kb < (int)nT; ++kb) {
            btrsm_kernel<<<dim3((unsigned)mt, ncn), 256, 0, st>>>(dBt, bb.dW, bb.dns, dms, d, q, kb);
            const int nc = (int)nT - kb - 1;
            if (nc > 0) bupdate_kernel<<<dim3((unsigned)(mt * nc), ncn), 256, 0, st>>>(dBt, bb.dA, bb.dns, dms, d, q, kb, mt);
        }
        if (cov) {
            bsyrk_cov_kernel<<<dim3((unsigned)(mt * mt), ncn), 256, 0, st>>>(dC, dBt, dms, Np, q, mt);
            bunpad_cov_kernel<<<dim3((unsigned)(mmax * ((mmax + 255) / 256)), ncn), 256, 0, st>>>(dC, dms, q, dU);
        } else {
            bvar_rows_kernel<<<dim3((unsigned)((mmax + 3) / 4), ncn), 256, 0, st>>>(dBt, bb.dks, dms, Np, q, dU);
        }
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[5], st));
        rc = batch_end_chunk(r, c0, cn, unc + (size_t)c0 * out_elems, dU, (size_t)cn * out_elems * 8, 2);
        if (rc) return rc;
    }
    batch_finish(r);
    return 0;
}

int tgp_gp_posterior_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                           const double *y, const double *yerr, const int64_t *ms, int64_t mmax, const double *Xs, int what,
                           double *alpha, double *unc, double *logdet, double *ydota, int32_t *info) {
    return posterior_batch(ctx, "tgp_gp_posterior_batch", nb, KSrc{ks, nullptr}, ns, nmax, X, y, yerr, ms, mmax, Xs, what, alpha, unc,
                           logdet, ydota, info);
}

int tgp_gp_posterior_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                               const double *y, const double *yerr, const int64_t *ms, int64_t mmax, const double *Xs, int what,
                               double *alpha, double *unc, double *logdet, double *ydota, int32_t *info) {
    return posterior_batch(ctx, "tgp_gp_posterior_batch_sum", nb, KSrc{nullptr, ks}, ns, nmax, X, y, yerr, ms, mmax, Xs, what, alpha,
                           unc, logdet, ydota, info);
}

// Bt_b <- L_b^-T for the `ncn` problems of a chunk, Bt_b holding the identity (S2f and S2g): the block substitution over the
// 128-column blocks kb; at step kb only the row tiles ti <= kb hold anything.  Bt_b is square: the "query rows" are the
// problem's own, ms = ns.
static void batch_subst_identity(hipStream_t st, double *dBt, const BatchBufs &bb, const BatchDims &d, unsigned ncn) {
    const int nT = (int)(d.Np / TGP_TB);
    const PostDims q{d.Np, 0};                                    // (mmax is not read by the substitution)
    for (int kb = 0; kb < nT; ++kb) {
        const int live = kb + 1;
        btrsm_kernel<<<dim3((unsigned)live, ncn), 256, 0, st>>>(dBt, bb.dW, bb.dns, bb.dns, d, q, kb);
        const int nc = nT - kb - 1;
        if (nc > 0) bupdate_kernel<<<dim3((unsigned)(live * nc), ncn), 256, 0, st>>>(dBt, bb.dA, bb.dns, bb.dns, d, q, kb, live);
    }
}

// ---- S2f: the likelihood gradient of every problem of S2e from its factor and alpha, in the same call ---------------------------
// Per chunk, after batch_factor_chunk with both sweeps: Bt_b <- identity, the block substitution Bt_b <- L_b^-T over the live row
// tiles, C_b = -Bt_b Bt_b^T over the lower tile pairs, the reduction against dK/dp and one fixed-order sum per problem.
// `any`: the entry of seam S2h, which takes the von Karman kinds too (one pair-sum launch per kernel class in the chunk).
// T: rows of `grad` per problem -- 1 for the entries of S2f / S2h, TGP_SUM_MAX for seam S2i, where the pair pass runs once per
// term over the problems whose term t has the launch's evaluator, into partial sums of their own, and the fixed-order
// reduction once per (problem, term); rows at or beyond a problem's term count are exactly 0.
static int solve_grad_batch(tgp_ctx *ctx, const char *fn, bool any, int T, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax,
                            const double *X, const double *y, const double *yerr, double *logdet, double *ydota, double *grad,
                            int32_t *info) {
    if (!ctx) return -1;
    if (!((ks.k1 || ks.ks) && ns && X && y && logdet && grad && info)) {
        ctx->err = std::string(fn) + ": ks, ns, X, y, logdet, grad and info must not be NULL";
        return -1;
    }
    BatchRun r;
    int rc = batch_begin(r, ctx, fn, nb, ks, ns, nmax, nullptr, logdet, ydota, info);
    if (rc) return rc;
    for (int b = 0; b < nb && !any; ++b)                    // (an unknown kind has been turned away by batch_begin)
        if (kind_to_ke(ks.k1[b].kind) != KE_GAUSS) {
            ctx->err = std::string(fn) + ": ks[" + std::to_string(b) + "].kind = " + std::to_string(ks.k1[b].kind) +
                       ": analytic derivatives exist for the Gaussian kernels only (RBF, AnisotropicRBF), as in the reference "
                       "(treegp/kernels.py:128-150)";
            return -1;
        }
    hipStream_t st = ctx->stream;
    const BatchDims &d = r.d;
    const int64_t Np = d.Np, nP = Np / TGP_PW, nT = Np / TGP_TB;
    const GradDims g{Np / 64, nP};
    // per problem beside S2e's arrays: Bt and C (Np x Np each), the reduction's partial sums and the four results per term
    rc = batch_arena(r, 2 * rup((size_t)Np * Np * 8) + rup((size_t)(T * g.nrb * g.nP) * 32) + rup((size_t)T * 32));
    if (rc) return rc;
    const int64_t C = r.C;
    BatchBufs &bb = r.bb;
    double *dBt = (double *)r.take((size_t)C * Np * Np * 8);
    double *dC = (double *)r.take((size_t)C * Np * Np * 8);
    double *dpart = (double *)r.take((size_t)C * T * g.nrb * g.nP * 32);
    double *dgrad = (double *)r.take((size_t)C * T * 32);

    for (int64_t c0 = 0; c0 < nb; c0 += C) {
        const int64_t cn = (nb - c0) < C ? (nb - c0) : C;
        const unsigned ncn = (unsigned)cn;
        rc = batch_factor_chunk(ctx, d, bb, c0, cn, ks, ns, nmax, X, y, yerr, true);
        if (rc) return rc;
        TGP_HIP(hipEventRecord(ctx->ev[4], st));
        bgrad_init_kernel<<<dim3((unsigned)(nT * nP), ncn), 256, 0, st>>>(dBt, dC, bb.dns, Np, (int)nP);
        batch_subst_identity(st, dBt, bb, d, ncn);
        bkinv_syrk_kernel<<<dim3((unsigned)(nT * (nT + 1) / 2), ncn), 256, 0, st>>>(dC, dBt, bb.dns, Np, (int)nP);
        const unsigned gw = (unsigned)(g.nrb * g.nP);
        // the pair pass's launch lists: for every term t, the problems with more than t terms by the evaluator of their term t,
        // each list in batch order (set t at t * cn of the table); one launch per list present
        int gcnt[TGP_SUM_MAX][3], gstart[TGP_SUM_MAX][3], tmax = 0;
        for (int t = 0; t < T; ++t) {
            int *gl = bb.hglist + (int64_t)t * cn;
            gcnt[t][0] = gcnt[t][1] = gcnt[t][2] = 0;
            for (int64_t b = 0; b < cn; ++b)
                if (t < bb.hks[b].nterms) ++gcnt[t][bb.hks[b].ke[t]];
            gstart[t][0] = 0;
            gstart[t][1] = gcnt[t][0];
            gstart[t][2] = gcnt[t][0] + gcnt[t][1];
            int fill[3] = {0, 0, 0};
            for (int64_t b = 0; b < cn; ++b)
                if (t < bb.hks[b].nterms) {
                    const int k = bb.hks[b].ke[t];
                    gl[gstart[t][k] + fill[k]++] = (int)b;
                }
            if (gcnt[t][0] + gcnt[t][1] + gcnt[t][2]) tmax = t + 1;
        }
        TGP_HIP(hipMemcpyAsync(bb.dglist, bb.hglist, (size_t)tmax * cn * 4, hipMemcpyHostToDevice, st));
        if (T > 1) TGP_HIP(hipMemsetAsync(dgrad, 0, (size_t)cn * T * 32, st));       // rows >= nterms_b: exactly 0
        for (int t = 0; t < tmax; ++t) {
            const int *gl = bb.dglist + (int64_t)t * cn;
#define TGP_PAIRS(KE, k)                                                                                                          \
            if (gcnt[t][k])                                                                                                           \
                bloglik_grad_kernel<KE><<<dim3(gw, gcnt[t][k]), 256, 0, st>>>(bb.dks, gl + gstart[t][k], t, T, bb.dns, bb.dX, bb.da, dC, Np, g, dpart);
            TGP_PAIRS(KE_GAUSS, 0)
            TGP_PAIRS(KE_VK, 1)
            TGP_PAIRS(KE_AVK, 2)
#undef TGP_PAIRS
        }
        bloglik_grad_reduce_kernel<<<dim3(ncn, (unsigned)tmax), 256, 0, st>>>(dpart, bb.dks, T, bb.dns, g, dgrad);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[5], st));
        rc = batch_end_chunk(r, c0, cn, grad + c0 * T * 4, dgrad, (size_t)cn * T * 32, 1);
        if (rc) return rc;
    }
    batch_finish(r);
    return 0;
}

int tgp_gp_solve_grad_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                            const double *y, const double *yerr, double *logdet, double *ydota, double *grad, int32_t *info) {
    return solve_grad_batch(ctx, "tgp_gp_solve_grad_batch", false, 1, nb, KSrc{ks, nullptr}, ns, nmax, X, y, yerr, logdet, ydota, grad, info);
}

int tgp_gp_solve_grad_batch_any(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                                const double *y, const double *yerr, double *logdet, double *ydota, double *grad, int32_t *info) {
    return solve_grad_batch(ctx, "tgp_gp_solve_grad_batch_any", true, 1, nb, KSrc{ks, nullptr}, ns, nmax, X, y, yerr, logdet, ydota, grad, info);
}

int tgp_gp_solve_grad_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                                const double *y, const double *yerr, double *logdet, double *ydota, double *grad, int32_t *info) {
    return solve_grad_batch(ctx, "tgp_gp_solve_grad_batch_sum", true, TGP_SUM_MAX, nb, KSrc{nullptr, ks}, ns, nmax, X, y, yerr, logdet,
                            ydota, grad, info);
}

// ---- S2g: diag(K^-1) of every problem of S2e from its factor, in the same call (leave-one-out, R&W 5.4.2) ----------------------
// Per chunk, after batch_factor_chunk: Bt_b <- identity, the block substitution Bt_b <- L_b^-T over the live row tiles (the
// launches of S2f), then one wave per row for |row i of Bt_b|^2 from the row's own panel on.  No C_b: half of S2f's flops behind
// the solve, one Np x Np buffer per problem.
static int loo_batch(tgp_ctx *ctx, const char *fn, int nb, const KSrc &ks, const int64_t *ns, int64_t nmax, const double *X,
                     const double *y, const double *yerr, double *alpha, double *invdiag, double *logdet, double *ydota, int32_t *info) {
    if (!ctx) return -1;
    if (!((ks.k1 || ks.ks) && ns && X && y && invdiag && logdet && info)) {
        ctx->err = std::string(fn) + ": ks, ns, X, y, invdiag, logdet and info must not be NULL";
        return -1;
    }
    BatchRun r;
    int rc = batch_begin(r, ctx, fn, nb, ks, ns, nmax, alpha, logdet, ydota, info);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const BatchDims &d = r.d;
    const int64_t Np = d.Np, nP = Np / TGP_PW, nT = Np / TGP_TB;
    // per problem beside S2e's arrays: Bt (Np x Np) and the diagonal in the caller's layout
    rc = batch_arena(r, rup((size_t)Np * Np * 8) + rup((size_t)nmax * 8));
    if (rc) return rc;
    const int64_t C = r.C;
    BatchBufs &bb = r.bb;
    double *dBt = (double *)r.take((size_t)C * Np * Np * 8);
    double *dD = (double *)r.take((size_t)C * nmax * 8);

    for (int64_t c0 = 0; c0 < nb; c0 += C) {
        const int64_t cn = (nb - c0) < C ? (nb - c0) : C;
        const unsigned ncn = (unsigned)cn;
        rc = batch_factor_chunk(ctx, d, bb, c0, cn, ks, ns, nmax, X, y, yerr, alpha != nullptr);
        if (rc) return rc;
        TGP_HIP(hipEventRecord(ctx->ev[4], st));
        binv_init_kernel<<<dim3((unsigned)(nT * nP), ncn), 256, 0, st>>>(dBt, bb.dns, Np, (int)nP);
        batch_subst_identity(st, dBt, bb, d, ncn);
        binv_diag_kernel<<<dim3((unsigned)((nmax + 3) / 4), ncn), 256, 0, st>>>(dBt, bb.dns, Np, nmax, dD);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[5], st));
        rc = batch_end_chunk(r, c0, cn, invdiag + c0 * nmax, dD, (size_t)cn * nmax * 8, 1);
        if (rc) return rc;
    }
    batch_finish(r);
    return 0;
}

int tgp_gp_loo_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X, const double *y,
                     const double *yerr, double *alpha, double *invdiag, double *logdet, double *ydota, int32_t *info) {
    return loo_batch(ctx, "tgp_gp_loo_batch", nb, KSrc{ks, nullptr}, ns, nmax, X, y, yerr, alpha, invdiag, logdet, ydota, info);
}

int tgp_gp_loo_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                         const double *y, const double *yerr, double *alpha, double *invdiag, double *logdet, double *ydota,
                         int32_t *info) {
    return loo_batch(ctx, "tgp_gp_loo_batch_sum", nb, KSrc{nullptr, ks}, ns, nmax, X, y, yerr, alpha, invdiag, logdet, ydota, info);
}
