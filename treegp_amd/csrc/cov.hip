// Posterior covariance (seam S3b): cov = k(Xs, Xs) - HT (K + D)^-1 HT^T  (treegp/gp_interp.py:184-192)
// and its diagonal alone, the posterior variance (seam S3c, further down)
// from the factor kept by tgp_gp_solve.  With Bt = HT L^-T (M x N) the result is
// Kss - Bt Bt^T, which reuses the factor instead of factorising a second time (the reference's
// own comment at gp_interp.py:189) and keeps the subtraction symmetric.
//
// Everything is the tuned NT MFMA tile of gemm_tile.h, so Bt and the covariance live in the same
// 256-wide panel layout as the factor (rows = query points, Mp x 256 per panel, ld 256):
//   right-looking block substitution over the 128-column blocks kb of L
//     Bt[:, kb]  = Bt[:, kb] W_kb^T                      (W_kb = inverse of the diagonal block)
//     Bt[:, c]  -= Bt[:, kb] L[c, kb]^T    for c > kb
//   cov = Kss - Bt Bt^T, one pass over all panels of Bt (run-time segment loop of the tile).
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "gemm_tile.h"
#include "post_tile.h"

namespace {
// out: panels of 256 columns, panel p at out + p * rows * 256, element (i, j) -> [i][j & 255]
template <int KE>
__global__ __launch_bounds__(256) void cross_panels_kernel(KParams p, const double *__restrict__ Xs, int64_t m,
                                                           const double *__restrict__ X, int64_t n, int self,
                                                           double *__restrict__ out, int64_t rows, int64_t ncols) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= ncols) return;
    out[panel_elem(i, j, rows)] = cross_value<KE>(p, Xs, m, X, n, self, i, j);
}

int launch_cross_panels(tgp_ctx *ctx, const tgp_kernel *k, const double *d_Xs, int64_t m, const double *d_X, int64_t n,
                        int self, double *d_out, int64_t rows, int64_t ncols) {
    const int ke = kind_to_ke(k->kind);
    TGP_ARG(ke >= 0 && rows <= 65535);
    const KParams p = make_kparams(k);
    dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)rows), block(256);
    switch (ke) {
        case KE_GAUSS: cross_panels_kernel<KE_GAUSS><<<grid, block, 0, ctx->stream>>>(p, d_Xs, m, d_X, n, self, d_out, rows, ncols); break;
        case KE_VK: cross_panels_kernel<KE_VK><<<grid, block, 0, ctx->stream>>>(p, d_Xs, m, d_X, n, self, d_out, rows, ncols); break;
        default: cross_panels_kernel<KE_AVK><<<grid, block, 0, ctx->stream>>>(p, d_Xs, m, d_X, n, self, d_out, rows, ncols); break;
    }
    TGP_HIP(hipGetLastError());
    return 0;
}

// Bt[:, kb] <- Bt[:, kb] W_kb^T      (one 128-row tile per workgroup)
__global__ __launch_bounds__(256, 2) void cov_trsm_kernel(double *Bk, const double *W) {
    const int64_t t = blockIdx.x;
    post_trsm_tile(Bk + t * TGP_TB * TGP_PW, W);
}

// Bt[:, c] -= Bt[:, kb] L[c, kb]^T for c = kb + 1 + blockIdx.y
// Bt holds the panels from pb on (panel p at Bt + (p - pb) * Mp * 256; pb = 0 but for tgp_factor_inv_diag's chunks)
__global__ __launch_bounds__(256, 2) void cov_update_kernel(double *Bt, int64_t Mp, const double *A, int64_t Np, int kb, int64_t pb) {
    post_update_tile(Bt, Mp, A, Np, kb, pb, blockIdx.x, kb + 1 + blockIdx.y);
}

// ---- the substitution in steps of S = 1024 (512) columns, with the factor's inverse slabs (trsv_big.hip) -------------------------
//   T  = Bt[:, K] V_K^T            (V_K = inverse of the S x S diagonal block: k <= j, 256-deep segments; out of place)
//   Bt[:, c] -= Bt[:, K] L[c, K]^T  for the tile columns c right of super-block K, ONE pass of depth 1024 on the DTV tile
// instead of eight dependent pairs of depth-128 launches per super-block.  Bt starts at panel pb, as in cov_update_kernel.
__global__ __launch_bounds__(256) void cov_diag_big_kernel(const double *__restrict__ Bt, int64_t Mp, const double *__restrict__ V,
                                                           int64_t Np, int64_t r0, int ncolt, double *__restrict__ T, int64_t pb) {
    const int ti = blockIdx.x / ncolt, tj = blockIdx.x % ncolt;          // 128-row tile of the queries, 128-column tile of the block
    const int64_t p0 = r0 >> 8;
    const double *a = Bt + (p0 - pb) * Mp * TGP_PW + (int64_t)ti * TGP_TB * TGP_PW;
    const double *b = V + (r0 + (int64_t)tj * TGP_TB) * TGP_PW;          // slab panel 0, rows r0 + 128 tj ..
    double *c = T + (int64_t)(tj >> 1) * Mp * TGP_PW + (int64_t)ti * TGP_TB * TGP_PW + (tj & 1) * TGP_TB;
    const int nseg = (tj >> 1) + 1;                                      // V_K is lower triangular: columns k <= j
    gemm_tile_128<0, TGP_PW, TGP_PW, TileDefault, 0>(a, b, c, nullptr, nullptr, nseg, Mp * TGP_PW, Np * TGP_PW);
}

template <int NS>                                                          // NS = S / 256 panels per super-block
__global__ __launch_bounds__(256, 2) void cov_update_big_kernel(double *Bt, int64_t Mp, const double *A, int64_t Np, int64_t r0,
                                                                int64_t pb) {
    const int64_t ti = blockIdx.x;
    const int64_t p0 = r0 >> 8;
    const int64_t c = (r0 >> 7) + 2 * NS + blockIdx.y;                   // global 128-tile column right of the super-block
    SegPtrs<NS> sp;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        sp.a[s] = Bt + (p0 + s - pb) * Mp * TGP_PW + ti * TGP_TB * TGP_PW;
        sp.b[s] = A + panel_off(p0 + s, Np) + (c * TGP_TB - (p0 + s) * TGP_PW) * TGP_PW;
    }
    double *cc = Bt + ((c >> 1) - pb) * Mp * TGP_PW + ti * TGP_TB * TGP_PW + (c & 1) * TGP_TB;
    gemm_tile_dtv_segs<4, TGP_PW, NS>(sp, cc);
}

// C(ti, tj) -= sum over all panels of Bt[ti] Bt[tj]^T        (C in the same panel layout, Mp rows)
__global__ __launch_bounds__(256, 2) void cov_syrk_kernel(double *Cpm, const double *Bt, int64_t Mp, int nP) {
    post_syrk_tile(Cpm, Bt, Mp, nP, blockIdx.x, blockIdx.y, 0);
}
}  // namespace

namespace {
// geometry + scratch shared by the entry points.  Covariance (var_rows == 0): Bt is Mp x Np, the result d_C Mp x Mp.
// Variance (var_rows > 0, seam S3c): Bt holds one chunk of Mp = var_rows query rows and there is no d_C; d_v and d_kss are Mp
// doubles each (the chunk's variances, the caller's k(x_i, x_i) of the dense route).  d_Xs holds all m query points either way.
// c0: first column of Bt that is stored (a multiple of the substitution's step): d_Bt holds the panels from c0 / 256 on and the
// substitution starts there.  0 but for the chunks of tgp_factor_inv_diag, whose columns left of c0 are known to be zero.
struct CovPlan {
    int64_t n, m, Np, Mp;
    int nP, nPm;
    double *d_X, *d_Xs, *d_Bt, *d_C, *d_v, *d_kss;
    int64_t c0 = 0;
};
int cov_plan(tgp_ctx *ctx, const tgp_factor *f, int64_t m, bool coords, CovPlan *pl, int64_t var_rows = 0, int cdim = 2) {   // cdim: columns of the coordinates
    pl->n = f->n; pl->m = m; pl->Np = f->Np;
    pl->nP = (int)(pl->Np / TGP_PW);
    pl->Mp = var_rows ? var_rows : (m + TGP_PW - 1) / TGP_PW * TGP_PW;   // 256: the covariance uses the panel layout too
    pl->nPm = (int)(pl->Mp / TGP_PW);
    TGP_ARG(pl->Mp <= 65535 && pl->Mp % TGP_PW == 0);
    const size_t tail = var_rows ? 2 * rup((size_t)pl->Mp * 8) : rup((size_t)pl->Mp * pl->Mp * 8);
    const size_t need = (coords ? rup((size_t)cdim * pl->n * 8) + rup((size_t)cdim * m * 8) : 0) + rup((size_t)pl->Mp * pl->Np * 8) + tail;
    int rc = tgp_ensure_scratch(ctx, need);
    if (rc) return rc;
    char *base = (char *)ctx->scratch;
    size_t off = 0;
    auto take = [&](size_t b) { char *p = base + off; off += rup(b); return (double *)p; };
    pl->d_X = coords ? take((size_t)cdim * pl->n * 8) : nullptr;
    pl->d_Xs = coords ? take((size_t)cdim * m * 8) : nullptr;
    pl->d_Bt = take((size_t)pl->Mp * pl->Np * 8);
    pl->d_C = var_rows ? nullptr : take((size_t)pl->Mp * pl->Mp * 8);
    pl->d_v = var_rows ? take((size_t)pl->Mp * 8) : nullptr;
    pl->d_kss = var_rows ? take((size_t)pl->Mp * 8) : nullptr;
    return 0;
}
// The substitution's step and the factor's inverse slabs: S = 1024 (512) with slabs (built on first use, factor_slabs), S = 0 for
// the 128-block substitution (below the big-step size, or TGP_COV_BIG=0).
int cov_step(tgp_ctx *ctx, tgp_factor *f, int *S, const double **slabs) {
    const bool no_big = getenv("TGP_COV_BIG") && atoi(getenv("TGP_COV_BIG")) == 0;     // A/B: the 128-block substitution
    *S = 0;
    *slabs = nullptr;
    if (!no_big) {
        int rc = factor_slabs(ctx, f, 1024, S, slabs);
        if (rc) return rc;
    }
    if (!((*S == 1024 || *S == 512) && *slabs)) *S = 0;
    return 0;
}
// Bt <- Bt L^-T by block substitution.  `tri`: row i of Bt starts as e_i (identity rows from c0 on: row tile t of Bt is global
// row tile c0 / 128 + t), so at the step that eliminates columns [r0, r0 + rows) only the row tiles above r0 + rows hold anything:
// the launches cover those tiles only (a third of the work).
int cov_substitute(tgp_ctx *ctx, tgp_factor *f, const CovPlan &pl, bool tri) {
    hipStream_t st = ctx->stream;
    const int nb = 2 * pl.nP;
    const unsigned mt = (unsigned)(pl.Mp / TGP_TB);
    const int64_t pb = pl.c0 >> 8;
    int S = 0;
    const double *slabs = nullptr;
    int rc = cov_step(ctx, f, &S, &slabs);
    if (rc) return rc;
    TGP_ARG(pl.c0 % (S ? S : TGP_PW) == 0);
    auto live = [&](int64_t end) {                          // row tiles that are not all zero before the step that ends at `end`
        const int64_t t = (end - pl.c0) / TGP_TB;
        return (unsigned)(t < (int64_t)mt ? t : (int64_t)mt);
    };
    if (S) {
        rc = tgp_ensure_scratch2(ctx, (size_t)pl.Mp * S * sizeof(double));
        if (rc) return rc;
        double *T = (double *)ctx->scratch2;
        for (int64_t r0 = pl.c0; r0 < pl.Np; r0 += S) {
            const int64_t rows = (pl.Np - r0) < S ? (pl.Np - r0) : S;
            const int ncolt = (int)(rows / TGP_TB);
            const unsigned mte = tri ? live(r0 + rows) : mt;
            cov_diag_big_kernel<<<mte * (unsigned)ncolt, 256, 0, st>>>(pl.d_Bt, pl.Mp, slabs, pl.Np, r0, ncolt, T, pb);
            for (int64_t q = 0; q < rows / TGP_PW; ++q)
                TGP_HIP(hipMemcpyAsync(pl.d_Bt + ((r0 >> 8) + q - pb) * pl.Mp * TGP_PW, T + q * pl.Mp * TGP_PW,
                                       (size_t)mte * TGP_TB * TGP_PW * sizeof(double), hipMemcpyDeviceToDevice, st));
            const int64_t right = (pl.Np - (r0 + rows)) / TGP_TB;
            if (right > 0 && S == 1024) cov_update_big_kernel<4><<<dim3(mte, (unsigned)right), 256, 0, st>>>(pl.d_Bt, pl.Mp, f->d_A, pl.Np, r0, pb);
            if (right > 0 && S == 512) cov_update_big_kernel<2><<<dim3(mte, (unsigned)right), 256, 0, st>>>(pl.d_Bt, pl.Mp, f->d_A, pl.Np, r0, pb);
        }
    } else {
        for (int kb = (int)(pl.c0 / TGP_TB); kb < nb; ++kb) {
            double *Bk = pl.d_Bt + ((int64_t)(kb >> 1) - pb) * pl.Mp * TGP_PW + (kb & 1) * TGP_TB;
            const unsigned mte = tri ? live((int64_t)(kb + 1) * TGP_TB) : mt;
            cov_trsm_kernel<<<mte, 256, 0, st>>>(Bk, f->d_W + (int64_t)kb * TGP_TB * TGP_TB);
            const int nc = nb - kb - 1;
            if (nc > 0) cov_update_kernel<<<dim3(mte, (unsigned)nc), 256, 0, st>>>(pl.d_Bt, pl.Mp, f->d_A, pl.Np, kb, pb);
        }
    }
    TGP_HIP(hipGetLastError());
    return 0;
}
// `cols` columns of `rows` rows between a row-major host array (ld `hld`) and 256-wide device panels of Mp rows: one 2D copy per
// panel, in panel order, on the context's stream
int copy_panels(tgp_ctx *ctx, hipMemcpyKind kind, const double *host, int64_t hld, int64_t rows, int64_t cols, double *dev,
                int64_t Mp) {
    for (int64_t p = 0; p * TGP_PW < cols; ++p) {
        const size_t w = (size_t)(cols - p * TGP_PW < TGP_PW ? cols - p * TGP_PW : TGP_PW) * 8;
        double *h = const_cast<double *>(host) + p * TGP_PW, *d = dev + p * Mp * TGP_PW;
        if (kind == hipMemcpyHostToDevice)
            TGP_HIP(hipMemcpy2DAsync(d, (size_t)TGP_PW * 8, h, (size_t)hld * 8, w, (size_t)rows, kind, ctx->stream));
        else
            TGP_HIP(hipMemcpy2DAsync(h, (size_t)hld * 8, d, (size_t)TGP_PW * 8, w, (size_t)rows, kind, ctx->stream));
    }
    return 0;
}
// d_Bt holds HT, d_C holds k(X2, X2), both in zero-padded panels: substitution, Kss - Bt Bt^T, result to the host
int cov_finish(tgp_ctx *ctx, tgp_factor *f, const CovPlan &pl, double *cov) {
    hipStream_t st = ctx->stream;
    const unsigned mt = (unsigned)(pl.Mp / TGP_TB);
    int rc = cov_substitute(ctx, f, pl, false);
    if (rc) return rc;
    cov_syrk_kernel<<<dim3(mt, mt), 256, 0, st>>>(pl.d_C, pl.d_Bt, pl.Mp, pl.nP);
    TGP_HIP(hipGetLastError());
    TGP_HIP(hipEventRecord(ctx->ev[1], st));
    rc = copy_panels(ctx, hipMemcpyDeviceToHost, cov, pl.m, pl.m, pl.m, pl.d_C, pl.Mp);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[2], st));
    TGP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->timings[3] = ms;                       // device compute
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
    ctx->timings[9] = ms;                       // (m, m) result to the caller's buffer
    return 0;
}
}  // namespace

extern "C" int tgp_gp_predict_cov(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                                  const double *Xs, int64_t m, double *cov) {
    TGP_ARG(f && k && X && Xs && cov && m > 0 && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CovPlan pl;
    int rc = cov_plan(ctx, f, m, true, &pl);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 2 * m * 8, hipMemcpyHostToDevice, st));
    // HT (gp_interp.py:177) and k(X2) (gp_interp.py:191), zero padded, in panels
    rc = launch_cross_panels(ctx, k, pl.d_Xs, m, pl.d_X, n, 0, pl.d_Bt, pl.Mp, pl.Np);
    if (rc) return rc;
    rc = launch_cross_panels(ctx, k, pl.d_Xs, m, pl.d_Xs, m, 1, pl.d_C, pl.Mp, pl.Mp);
    if (rc) return rc;
    return cov_finish(ctx, f, pl, cov);
}

// The same with HT = kernel(X2, Y=X1) (m, n) and Kss = kernel(X2) (m, m) evaluated by the caller (row-major host arrays):
// any scikit-learn kernel tree (gp_interp.py:184-192 with the factor kept by tgp_gp_solve_dense).
extern "C" int tgp_gp_predict_cov_dense(tgp_ctx *ctx, tgp_factor *f, const double *HT, const double *Kss, int64_t m, double *cov) {
    TGP_ARG(f && HT && Kss && cov && m > 0);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CovPlan pl;
    int rc = cov_plan(ctx, f, m, false, &pl);
    if (rc) return rc;
    const int64_t n = f->n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemsetAsync(pl.d_Bt, 0, (size_t)pl.Mp * pl.Np * 8, st));
    TGP_HIP(hipMemsetAsync(pl.d_C, 0, (size_t)pl.Mp * pl.Mp * 8, st));
    rc = copy_panels(ctx, hipMemcpyHostToDevice, HT, n, m, n, pl.d_Bt, pl.Mp);
    if (rc) return rc;
    rc = copy_panels(ctx, hipMemcpyHostToDevice, Kss, m, m, m, pl.d_C, pl.Mp);
    if (rc) return rc;
    return cov_finish(ctx, f, pl, cov);
}

// ---- posterior variance (seam S3c): var_i = k(x_i, x_i) - |Bt_i|^2, the diagonal of the covariance above without forming it ----
// Callers of the reference take np.diag of the covariance and nothing else.  The query points go through in chunks of Mc rows:
// HT of the chunk into Bt, the same substitution as the covariance (cov_substitute, unchanged), then one pass of
// var_rows_kernel over the chunk's Bt.  No M x M buffer, so m is not bounded by the covariance's 65 535.  Rows of Bt do not
// depend on the rows around them and var_rows_kernel sums in a fixed order, so the result does not depend on Mc.
#ifndef TGP_VAR_CHUNK_DEFAULT
#define TGP_VAR_CHUNK_DEFAULT 16384   // rows per chunk (LAB_NOTES.md: 4096 - 32 768 measured)
#endif
namespace {
// one wave per query row (row_sqnorm_wave)
__global__ __launch_bounds__(256) void var_rows_kernel(const double *__restrict__ Bt, int64_t Mp, int nP, int64_t rows,
                                                       const double *__restrict__ kss, double amp, double *__restrict__ var) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;                                       // whole waves leave together
    const double acc = row_sqnorm_wave(Bt, Mp, nP, i);
    if (lane == 0) var[i] = (kss ? kss[i] : amp) - acc;
}

// rows per chunk: TGP_VAR_CHUNK (rounded up to 256) or the default, at most TGP_VAR_CHUNK_MAX, and at most what keeps the
// chunk's Bt (Mc x Np) plus the substitution's staging (Mc x 1024, scratch2) within half of the device memory that is free or
// already held as scratch by this context; never more than m needs
int var_chunk_rows(tgp_ctx *ctx, const tgp_factor *f, int64_t m, int64_t *Mc) {
    int64_t want = TGP_VAR_CHUNK_DEFAULT;
    const char *e = getenv("TGP_VAR_CHUNK");                     // read per call (tests, A/B runs), as TGP_COV_BIG is
    if (e && atoll(e) > 0) want = (atoll(e) + TGP_PW - 1) / TGP_PW * TGP_PW;
    if (want > TGP_VAR_CHUNK_MAX) want = TGP_VAR_CHUNK_MAX;
    size_t fr = 0, tot = 0;
    TGP_HIP(hipMemGetInfo(&fr, &tot));
    const double avail = (double)fr + (double)ctx->scratch_bytes + (double)ctx->scratch2_bytes;
    int64_t cap = (int64_t)(0.5 * avail / ((double)(f->Np + 1024) * sizeof(double))) / TGP_PW * TGP_PW;
    if (cap < TGP_PW) cap = TGP_PW;
    const int64_t need = (m + TGP_PW - 1) / TGP_PW * TGP_PW;
    *Mc = want < cap ? want : cap;
    if (need < *Mc) *Mc = need;
    return 0;
}

// HT of every chunk is written into pl.d_Bt by `fill` (rows r0 .. r0 + rows of the queries, Mp rows of panels, zero padded),
// the dense route's k(x_i, x_i) into pl.d_kss; then substitution, norms, the chunk's variances to var + r0.
// `tri` (tgp_factor_inv_diag): the chunk's rows are the identity's from column r0 on, so it stores and sums those panels only.
// Timings: [3] device compute, [9] transfer of the result, each summed over the chunks.
template <class Fill>
int var_chunks(tgp_ctx *ctx, tgp_factor *f, CovPlan &pl, int64_t Mc, double amp, bool dense, bool tri, double *var, Fill fill) {
    hipStream_t st = ctx->stream;
    double t_dev = 0.0, t_d2h = 0.0;
    for (int64_t r0 = 0; r0 < pl.m; r0 += Mc) {
        const int64_t rows = (pl.m - r0) < Mc ? (pl.m - r0) : Mc;
        CovPlan cp = pl;
        cp.Mp = (rows + TGP_PW - 1) / TGP_PW * TGP_PW;          // a short last chunk substitutes only the rows it has
        cp.nPm = (int)(cp.Mp / TGP_PW);
        cp.c0 = tri ? r0 : 0;
        const int np = cp.nP - (int)(cp.c0 >> 8);               // panels the chunk stores
        if (r0 > 0) TGP_HIP(hipEventRecord(ctx->ev[0], st));     // (the first chunk's interval starts before the uploads)
        int rc = fill(cp, r0, rows, np);
        if (rc) return rc;
        rc = cov_substitute(ctx, f, cp, tri);
        if (rc) return rc;
        var_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(cp.d_Bt, cp.Mp, np, rows, dense ? cp.d_kss : nullptr, amp, cp.d_v);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[1], st));
        TGP_HIP(hipMemcpyAsync(var + r0, cp.d_v, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipEventRecord(ctx->ev[2], st));
        TGP_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        t_dev += ms;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        t_d2h += ms;
    }
    ctx->timings[3] = t_dev;                    // device compute
    ctx->timings[9] = t_d2h;                    // (m) result to the caller's buffer
    return 0;
}
}  // namespace

extern "C" int tgp_gp_predict_var(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                                  const double *Xs, int64_t m, double *var) {
    TGP_ARG(f && k && X && Xs && var && m > 0 && n == f->n);
    TGP_ARG(kind_to_ke(k->kind) >= 0);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t Mc = 0;
    int rc = var_chunk_rows(ctx, f, m, &Mc);
    if (rc) return rc;
    CovPlan pl;
    rc = cov_plan(ctx, f, m, true, &pl, Mc);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 2 * m * 8, hipMemcpyHostToDevice, st));
    // k(x_i, x_i) of the four parametrised kinds is exactly amp (the self kernel's diagonal, tgp_kernel_matrix)
    return var_chunks(ctx, f, pl, Mc, k->amp, false, false, var, [&](const CovPlan &cp, int64_t r0, int64_t rows, int) {
        return launch_cross_panels(ctx, k, cp.d_Xs + 2 * r0, rows, cp.d_X, n, 0, cp.d_Bt, cp.Mp, cp.Np);
    });
}

// ---- S3b / S3c in three dimensions: the two entries above with (n, 3) coordinates and the cross panels of nd3.hip; substitution,
// products and row norms are the same launches, so var3 is the diagonal of cov3 as var is of cov
extern "C" int tgp_gp_predict_cov3(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel3 *k, const double *X, int64_t n,
                                   const double *Xs, int64_t m, double *cov) {
    if (tgp_kernel3_check(ctx, k, "tgp_gp_predict_cov3")) return -1;
    TGP_ARG(f && X && Xs && cov && m > 0 && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CovPlan pl;
    int rc = cov_plan(ctx, f, m, true, &pl, 0, 3);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 3 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 3 * m * 8, hipMemcpyHostToDevice, st));
    rc = launch_cross_panels3(ctx, k, pl.d_Xs, m, pl.d_X, n, 0, pl.d_Bt, pl.Mp, pl.Np);
    if (rc) return rc;
    rc = launch_cross_panels3(ctx, k, pl.d_Xs, m, pl.d_Xs, m, 1, pl.d_C, pl.Mp, pl.Mp);
    if (rc) return rc;
    return cov_finish(ctx, f, pl, cov);
}

extern "C" int tgp_gp_predict_var3(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel3 *k, const double *X, int64_t n,
                                   const double *Xs, int64_t m, double *var) {
    if (tgp_kernel3_check(ctx, k, "tgp_gp_predict_var3")) return -1;
    TGP_ARG(f && X && Xs && var && m > 0 && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t Mc = 0;
    int rc = var_chunk_rows(ctx, f, m, &Mc);
    if (rc) return rc;
    CovPlan pl;
    rc = cov_plan(ctx, f, m, true, &pl, Mc, 3);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 3 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 3 * m * 8, hipMemcpyHostToDevice, st));
    return var_chunks(ctx, f, pl, Mc, k->amp, false, false, var, [&](const CovPlan &cp, int64_t r0, int64_t rows, int) {
        return launch_cross_panels3(ctx, k, cp.d_Xs + 3 * r0, rows, cp.d_X, n, 0, cp.d_Bt, cp.Mp, cp.Np);
    });
}

// The same with HT = kernel(X2, Y=X1) (m, n) and kss = kernel.diag(X2) (m) evaluated by the caller (host arrays).
extern "C" int tgp_gp_predict_var_dense(tgp_ctx *ctx, tgp_factor *f, const double *HT, const double *kss, int64_t m, double *var) {
    TGP_ARG(f && HT && kss && var && m > 0);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t Mc = 0;
    int rc = var_chunk_rows(ctx, f, m, &Mc);
    if (rc) return rc;
    CovPlan pl;
    rc = cov_plan(ctx, f, m, false, &pl, Mc);
    if (rc) return rc;
    const int64_t n = f->n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    return var_chunks(ctx, f, pl, Mc, 0.0, true, false, var, [&](const CovPlan &cp, int64_t r0, int64_t rows, int) -> int {
        TGP_HIP(hipMemsetAsync(cp.d_Bt, 0, (size_t)cp.Mp * cp.Np * 8, st));
        int rc = copy_panels(ctx, hipMemcpyHostToDevice, HT + r0 * n, n, rows, n, cp.d_Bt, cp.Mp);
        if (rc) return rc;
        TGP_HIP(hipMemcpyAsync(cp.d_kss, kss + r0, (size_t)rows * 8, hipMemcpyHostToDevice, st));
        return 0;
    });
}

// ---- diag(K^-1) from a kept factor (seam S3e): d_i = |L^-1 e_i|^2, row i of Bt = E L^-T -------------------------------------
// The leave-one-out quantities of a GP (Rasmussen & Williams 5.4.2) need alpha = K^-1 r and this diagonal.  Identity rows go
// through the substitution above in chunks [r0, r0 + R), r0 and R multiples of its step (1024 with the inverse slabs, 256 on
// the 128-block path; the chunks lie on the factor's own super-block grid).  Row i of Bt is zero left of column i, so a chunk
// stores and updates only the panels from r0 on (R x (Np - r0) doubles), its substitution starts at the super-block r0 and, as
// for the gradient's L^-T, launches only the row tiles that are not all zero yet (`tri`).  Work sum_chunks R (N - r0)^2 at most,
// ~N^3 / 3 flops with the row-tile pruning.  The squared row norms are var_rows_kernel's (one wave per row, fixed order, no
// atomics): rows do not depend on the rows around them, and the zeros a larger chunk carries left of r0 add exact zeros, so the
// result does not depend on the chunk size.
#ifndef TGP_INVDIAG_CHUNK_DEFAULT
#define TGP_INVDIAG_CHUNK_DEFAULT 16384   // identity rows per chunk (LAB_NOTES.md: 4096 - 16 384 measured)
#endif
namespace {
// rows [c0, c0 + Mp) of the identity into a chunk's panels (from panel c0 / 256 on, zeroed before)
__global__ __launch_bounds__(256) void ident_chunk_kernel(double *Bt, int64_t Mp, int64_t c0) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= Mp) return;
    const int64_t i = c0 + li;
    Bt[panel_elem(li, i, Mp) - (c0 >> 8) * Mp * TGP_PW] = 1.0;
}

// rows per chunk: TGP_INVDIAG_CHUNK (rounded up to the step) or the default, at most the largest multiple of the step that the
// row grids accept, at most what keeps the chunk (R x Np) and the substitution's staging (R x 1024) within half of the device
// memory that is free or already held as scratch by this context; never more than n needs
int inv_diag_chunk_rows(tgp_ctx *ctx, const tgp_factor *f, int64_t step, int64_t *R) {
    int64_t want = TGP_INVDIAG_CHUNK_DEFAULT;
    const char *e = getenv("TGP_INVDIAG_CHUNK");                 // read per call (tests, A/B runs)
    if (e && atoll(e) > 0) want = atoll(e);
    want = (want + step - 1) / step * step;
    const int64_t most = TGP_VAR_CHUNK_MAX / step * step;
    if (want > most) want = most;
    size_t fr = 0, tot = 0;
    TGP_HIP(hipMemGetInfo(&fr, &tot));
    const double avail = (double)fr + (double)ctx->scratch_bytes + (double)ctx->scratch2_bytes;
    int64_t cap = (int64_t)(0.5 * avail / ((double)(f->Np + 1024) * sizeof(double))) / step * step;
    if (cap < step) cap = step;
    const int64_t need = (f->n + step - 1) / step * step;
    *R = want < cap ? want : cap;
    if (need < *R) *R = need;
    return 0;
}
}  // namespace

extern "C" int tgp_factor_inv_diag(tgp_ctx *ctx, tgp_factor *f, double *d) {
    TGP_ARG(f && d && f->n > 0);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = f->n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));                   // (the first chunk's interval includes building the slabs)
    int S = 0;
    const double *slabs = nullptr;
    int rc = cov_step(ctx, f, &S, &slabs);
    if (rc) return rc;
    const int64_t step = S ? S : TGP_PW;
    int64_t R = 0;
    rc = inv_diag_chunk_rows(ctx, f, step, &R);
    if (rc) return rc;
    CovPlan pl;
    rc = cov_plan(ctx, f, n, false, &pl, R < f->Np ? R : f->Np);   // d_Bt: the first chunk, at most Np x Np
    if (rc) return rc;
    // kss = nullptr, amp = 0: var_rows_kernel leaves 0 - |row|^2, negated exactly on the host
    rc = var_chunks(ctx, f, pl, R, 0.0, false, true, d, [&](const CovPlan &cp, int64_t r0, int64_t, int np) -> int {
        TGP_HIP(hipMemsetAsync(cp.d_Bt, 0, (size_t)cp.Mp * np * TGP_PW * 8, st));
        ident_chunk_kernel<<<(unsigned)(cp.Mp / 256), 256, 0, st>>>(cp.d_Bt, cp.Mp, r0);
        return 0;
    });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) d[i] = -d[i];
    return 0;
}

// ---- diagonal blocks of K^-1 from a kept factor (seam S3h): P_GG = Bt_G Bt_G^T for groups G of contiguous rows ------------------
// What leaving a GROUP of points out of a GP needs (Rasmussen & Williams 5.4.2 with blocks for points).  The rows of Bt = E L^-T
// are made exactly as for tgp_factor_inv_diag (ident_chunk_kernel, cov_substitute with `tri`, both substitutions); where that
// keeps the squared norm of every row, this keeps the Gram matrix of every group's rows.  A chunk starts at the largest multiple
// of the substitution's step at or below the first row of the first group that is not done and finishes every group that lies
// wholly inside it, so a group never straddles two chunks (at most step - 1 rows and one partial group are substituted twice per
// chunk); the chunk is TGP_INVDIAG_CHUNK rows or its default, raised to the largest group plus one step where that is more.
// Per chunk: one launch of the fp64 MFMA tile product over the lower tile pairs of every finished group's 128-row tiles
// (global tiles: a group that starts or ends inside one uses the tiles that cover it), every sum from the panel that holds the
// group's first row -- left of it those rows are zero, and a chunk that begins there does not even store them -- then one
// launch that drops the rows outside the groups, negates and mirrors the lower triangles into the row-major blocks.  No
// atomics; an entry's terms and their order depend on its group alone: neither on the chunk size nor on the other groups.
// Memory beside the chunk's Bt: 128 KiB per tile pair and the chunk's blocks (sum of g^2 doubles), in the context's io buffer.
namespace {
__global__ __launch_bounds__(256, 2) void inv_blocks_syrk_kernel(double *C, const double *Bt, int64_t Mp, const InvBlockItem *items) {
    inv_block_syrk_tile(C, Bt, Mp, items, blockIdx.x);
}
__global__ __launch_bounds__(256) void inv_blocks_write_kernel(const double *C, const InvBlockItem *items, double *out) {
    inv_block_write_tile(C, items, blockIdx.x, out);
}

struct InvBlockChunk {
    int64_t c0, rows;            // first row (a multiple of the step) and rows substituted
    int64_t item0, nitems;       // its tile pairs in the item table
    int64_t out0, outlen;        // its groups' blocks in the caller's array (doubles)
};

int inv_blocks_check(tgp_ctx *ctx, const tgp_factor *f, const int64_t *starts, int64_t ngroups, const double *blocks) {
    static const std::string fn = "tgp_factor_inv_blocks: ";
    auto s = [](int64_t v) { return std::to_string((long long)v); };
    if (!(f && starts && blocks)) { ctx->err = fn + "f, starts and blocks must not be NULL"; return -1; }
    if (ngroups < 1) { ctx->err = fn + "ngroups = " + s(ngroups) + " must be >= 1"; return -1; }
    if (starts[0] != 0) { ctx->err = fn + "starts[0] = " + s(starts[0]) + " must be 0"; return -1; }
    for (int64_t g = 0; g < ngroups; ++g) {
        if (starts[g + 1] <= starts[g]) {
            ctx->err = fn + "starts[" + s(g + 1) + "] = " + s(starts[g + 1]) + " is not above starts[" + s(g) + "] = " + s(starts[g]);
            return -1;
        }
        if (starts[g + 1] - starts[g] > TGP_INVBLOCK_GMAX) {
            ctx->err = fn + "group " + s(g) + " (starts[" + s(g) + "] = " + s(starts[g]) + " to starts[" + s(g + 1) + "] = " +
                       s(starts[g + 1]) + ") has more than TGP_INVBLOCK_GMAX = " + s(TGP_INVBLOCK_GMAX) + " rows";
            return -1;
        }
    }
    if (starts[ngroups] != f->n) {
        ctx->err = fn + "starts[" + s(ngroups) + "] = " + s(starts[ngroups]) + " must be the factor's n = " + s(f->n);
        return -1;
    }
    return 0;
}

// the chunks and the tile pairs of every group (host only).  R: rows per chunk, a multiple of `step`, at least the largest group
// plus step - 1 unless it covers all n rows
void inv_blocks_layout(const int64_t *starts, int64_t ngroups, int64_t n, int64_t Np, int64_t step, int64_t R,
                       std::vector<InvBlockChunk> *chunks, std::vector<InvBlockItem> *items) {
    const int nP = (int)(Np / TGP_PW);
    int64_t g = 0, out = 0;
    while (g < ngroups) {
        InvBlockChunk ch;
        ch.c0 = starts[g] / step * step;
        ch.rows = (n - ch.c0) < R ? (n - ch.c0) : R;
        ch.item0 = (int64_t)items->size();
        ch.out0 = out;
        const int64_t pb = ch.c0 >> 8;
        int64_t local = 0;
        for (; g < ngroups && starts[g + 1] <= ch.c0 + ch.rows; ++g) {
            const int64_t ls = starts[g] - ch.c0, le = starts[g + 1] - ch.c0, gs = le - ls;
            const int64_t t0 = ls / TGP_TB, t1 = (le - 1) / TGP_TB;
            for (int64_t ti = t0; ti <= t1; ++ti)
                for (int64_t tj = t0; tj <= ti; ++tj) {
                    InvBlockItem it;
                    it.ta = (int)ti; it.tb = (int)tj;
                    it.p0 = (int)((starts[g] >> 8) - pb);
                    it.nseg = nP - (int)(starts[g] >> 8);
                    it.ra = (int)(ti * TGP_TB - ls); it.rb = (int)(tj * TGP_TB - ls);
                    it.g = (int)gs; it.pad = 0;
                    it.out = local;
                    items->push_back(it);
                }
            local += gs * gs;
        }
        ch.nitems = (int64_t)items->size() - ch.item0;
        ch.outlen = local;
        out += local;
        chunks->push_back(ch);
    }
}
}  // namespace

extern "C" int tgp_factor_inv_blocks(tgp_ctx *ctx, tgp_factor *f, const int64_t *starts, int64_t ngroups, double *blocks) {
    if (!ctx) return -1;
    int rc = inv_blocks_check(ctx, f, starts, ngroups, blocks);
    if (rc) return rc;
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = f->n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));                   // (the first chunk's interval includes building the slabs)
    int S = 0;
    const double *slabs = nullptr;
    rc = cov_step(ctx, f, &S, &slabs);
    if (rc) return rc;
    const int64_t step = S ? S : TGP_PW;
    int64_t R = 0, gmax = 0;
    rc = inv_diag_chunk_rows(ctx, f, step, &R);
    if (rc) return rc;
    for (int64_t g = 0; g < ngroups; ++g) gmax = starts[g + 1] - starts[g] > gmax ? starts[g + 1] - starts[g] : gmax;
    const int64_t fits = (gmax + 2 * step - 1) / step * step;  // a group that starts step - 1 rows into its chunk still ends inside
    if (R < fits) R = fits;
    std::vector<InvBlockChunk> chunks;
    std::vector<InvBlockItem> items;
    inv_blocks_layout(starts, ngroups, n, f->Np, step, R, &chunks, &items);
    int64_t most_items = 0, most_out = 0;
    for (const InvBlockChunk &ch : chunks) {
        most_items = ch.nitems > most_items ? ch.nitems : most_items;
        most_out = ch.outlen > most_out ? ch.outlen : most_out;
    }
    CovPlan pl;
    rc = cov_plan(ctx, f, n, false, &pl, R < f->Np ? R : f->Np);   // d_Bt: the largest chunk, at most Np x Np
    if (rc) return rc;
    // io buffer: the item table | the tile slots of one chunk (an even number: two per strip) | one chunk's blocks
    const size_t tab_bytes = rup(items.size() * sizeof(InvBlockItem));
    const size_t slot_bytes = rup((size_t)((most_items + 1) / 2) * TGP_TB * TGP_PW * sizeof(double));
    rc = tgp_ensure_io(ctx, tab_bytes + slot_bytes + rup((size_t)most_out * sizeof(double)));
    if (rc) return rc;
    InvBlockItem *d_items = (InvBlockItem *)tgp_io_buffer(ctx);
    double *d_C = (double *)((char *)tgp_io_buffer(ctx) + tab_bytes);
    double *d_out = (double *)((char *)d_C + slot_bytes);
    void *pin = nullptr;
    rc = tgp_ensure_pinned(ctx, items.size() * sizeof(InvBlockItem), &pin);
    if (rc) return rc;
    memcpy(pin, items.data(), items.size() * sizeof(InvBlockItem));
    TGP_HIP(hipMemcpyAsync(d_items, pin, items.size() * sizeof(InvBlockItem), hipMemcpyHostToDevice, st));
    double t_dev = 0.0, t_d2h = 0.0;
    bool first = true;
    for (const InvBlockChunk &ch : chunks) {
        CovPlan cp = pl;
        cp.Mp = (ch.rows + TGP_PW - 1) / TGP_PW * TGP_PW;
        cp.nPm = (int)(cp.Mp / TGP_PW);
        cp.c0 = ch.c0;
        const int np = cp.nP - (int)(cp.c0 >> 8);               // panels the chunk stores
        if (!first) TGP_HIP(hipEventRecord(ctx->ev[0], st));
        first = false;
        TGP_HIP(hipMemsetAsync(cp.d_Bt, 0, (size_t)cp.Mp * np * TGP_PW * 8, st));
        ident_chunk_kernel<<<(unsigned)(cp.Mp / 256), 256, 0, st>>>(cp.d_Bt, cp.Mp, cp.c0);
        rc = cov_substitute(ctx, f, cp, true);
        if (rc) return rc;
        TGP_HIP(hipMemsetAsync(d_C, 0, (size_t)((ch.nitems + 1) / 2) * TGP_TB * TGP_PW * sizeof(double), st));
        inv_blocks_syrk_kernel<<<(unsigned)ch.nitems, 256, 0, st>>>(d_C, cp.d_Bt, cp.Mp, d_items + ch.item0);
        inv_blocks_write_kernel<<<(unsigned)ch.nitems, 256, 0, st>>>(d_C, d_items + ch.item0, d_out);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[1], st));
        TGP_HIP(hipMemcpyAsync(blocks + ch.out0, d_out, (size_t)ch.outlen * 8, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipEventRecord(ctx->ev[2], st));
        TGP_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        t_dev += ms;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        t_d2h += ms;
    }
    ctx->timings[3] = t_dev;                    // device compute
    ctx->timings[9] = t_d2h;                    // the blocks to the caller's buffer
    return 0;
}

// ---- gradient of the log marginal likelihood (kernel derivative convention of treegp/kernels.py:128-150) ------------
//   dlogL/dp = 1/2 sum_ij (alpha_i alpha_j - [K^-1]_ij) dK_ij/dp
// for the four numbers a Gaussian kernel is made of on the device: p = log amp, a, b, c (invLam 00, 01 = 10, 11); the chain rule
// from there to theta stays on the host (kernels.spec_jacobian: the dInvLam/dtheta matrices of kernels.py:138-145).
// K^-1 = L^-T L^-1 comes from the substitution above started at the identity: Bt = L^-T is upper triangular, so both the
// substitution and the product Bt Bt^T skip what is known to be zero (2/3 N^3 flops together, twice a factorisation), and the
// sum over (i, j) is one pass over the lower triangle with dK/dp evaluated from the coordinates.
namespace {
__global__ __launch_bounds__(256) void ident_panels_kernel(double *Bt, int64_t Mp, int64_t Np) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Np) Bt[panel_elem(i, i, Mp)] = 1.0;
}

// lower tile pairs (ti >= tj), linear in blockIdx.x:  C(ti, tj) = -sum_{p >= ti / 2} Bt[ti][p] Bt[tj][p]^T   (C zero before)
__global__ __launch_bounds__(256, 2) void kinv_syrk_kernel(double *Cpm, const double *Bt, int64_t Mp, int nP) {
    int64_t ti, tj;
    tri_index(blockIdx.x, ti, tj);
    post_syrk_tile(Cpm, Bt, Mp, nP, ti, tj, ti >> 1);               // row tile ti of L^-T is zero left of its own panel
}

// 64 rows x one 256-column panel per workgroup over the lower triangle; four partial sums per workgroup
template <int KE>
__global__ __launch_bounds__(256) void loglik_grad_kernel(KParams p, const double *__restrict__ X, const double *__restrict__ alpha,
                                                          const double *__restrict__ Cpm, int64_t Mp, int64_t n,
                                                          double *__restrict__ partial) {
    loglik_grad_block<KE>(p, X, alpha, Cpm, Mp, n, blockIdx.x, (int64_t)blockIdx.y * 64,
                          partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// fixed-order sum of the workgroups' partial sums (one workgroup: the result does not depend on the schedule)
__global__ __launch_bounds__(256) void loglik_grad_reduce_kernel(const double *__restrict__ partial, int64_t count, double *__restrict__ out) {
    loglik_grad_reduce(partial, count, 1, 1, out);          // the partial sums are dense: one run of `count`, read in order
}
}  // namespace

// d_X (2 n) and d_alpha (n) on the device; grad: 4 doubles on the host.  Synchronises the stream.
int launch_loglik_grad(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *d_X, const double *d_alpha, double *grad) {
    hipStream_t st = ctx->stream;
    const int64_t n = f->n;
    CovPlan pl;
    int rc = cov_plan(ctx, f, n, false, &pl);             // m = n: d_Bt (Np x Np) <- L^-T, d_C (Np x Np) <- -K^-1
    if (rc) return rc;
    const int64_t nrb = (n + 63) / 64;
    const int64_t nparts = nrb * pl.nP;
    rc = tgp_ensure_scratch2(ctx, (size_t)(nparts * 4 + 4) * sizeof(double) > (size_t)pl.Mp * 1024 * sizeof(double)
                                      ? (size_t)(nparts * 4 + 4) * sizeof(double) : (size_t)pl.Mp * 1024 * sizeof(double));
    if (rc) return rc;
    TGP_HIP(hipMemsetAsync(pl.d_Bt, 0, (size_t)pl.Mp * pl.Np * 8, st));
    TGP_HIP(hipMemsetAsync(pl.d_C, 0, (size_t)pl.Mp * pl.Mp * 8, st));
    ident_panels_kernel<<<(unsigned)(pl.Np / 256), 256, 0, st>>>(pl.d_Bt, pl.Mp, pl.Np);
    rc = cov_substitute(ctx, f, pl, true);
    if (rc) return rc;
    const int64_t mt = pl.Mp / TGP_TB;
    kinv_syrk_kernel<<<(unsigned)(mt * (mt + 1) / 2), 256, 0, st>>>(pl.d_C, pl.d_Bt, pl.Mp, pl.nP);
    double *partial = (double *)ctx->scratch2;             // the substitution's staging buffer is free again
    const dim3 grid((unsigned)pl.nP, (unsigned)nrb);
    switch (kind_to_ke(k->kind)) {                          // the callers have checked the kind
        case KE_GAUSS: loglik_grad_kernel<KE_GAUSS><<<grid, 256, 0, st>>>(make_kparams(k), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
        case KE_VK: loglik_grad_kernel<KE_VK><<<grid, 256, 0, st>>>(make_kparams(k), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
        default: loglik_grad_kernel<KE_AVK><<<grid, 256, 0, st>>>(make_kparams(k), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
    }
    loglik_grad_reduce_kernel<<<1, 256, 0, st>>>(partial, nparts, partial + nparts * 4);
    TGP_HIP(hipGetLastError());
    TGP_HIP(hipEventRecord(ctx->ev[4], st));
    TGP_HIP(hipMemcpyAsync(grad, partial + nparts * 4, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    TGP_HIP(hipStreamSynchronize(st));
    return 0;
}

static int loglik_grad_kind_check(tgp_ctx *ctx, const tgp_kernel *k) {
    if (kind_to_ke(k->kind) == KE_GAUSS) return 0;
    ctx->err = "tgp_gp_loglik_grad: analytic derivatives exist for the Gaussian kernels only (RBF, AnisotropicRBF), as in the "
               "reference (treegp/kernels.py:128-150)";
    return -1;
}

static int loglik_grad_known_kind(tgp_ctx *ctx, const tgp_kernel *k, const char *fn) {
    if (kind_to_ke(k->kind) >= 0) return 0;
    ctx->err = std::string(fn) + ": unknown kernel kind " + std::to_string(k->kind);
    return -1;
}

static int loglik_grad_from_host(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n, const double *alpha,
                                 double *grad) {
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = tgp_ensure_io(ctx, (size_t)3 * n * sizeof(double));          // coordinates and alpha: outside the scratch areas
    if (rc) return rc;
    double *d_X = (double *)tgp_io_buffer(ctx), *d_alpha = d_X + 2 * n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(d_alpha, alpha, n * 8, hipMemcpyHostToDevice, st));
    rc = launch_loglik_grad(ctx, f, k, d_X, d_alpha, grad);
    if (rc) return rc;
    float ms = 0.f;
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[4]));
    ctx->timings[3] = ms;
    return 0;
}

extern "C" int tgp_gp_loglik_grad(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n, const double *alpha,
                                  double *grad) {
    TGP_ARG(f && k && X && alpha && grad && n == f->n);
    if (loglik_grad_kind_check(ctx, k)) return -1;
    return loglik_grad_from_host(ctx, f, k, X, n, alpha, grad);
}

// S2h: the same for every kind (the von Karman kinds through loglik_grad_block<KE_VK / KE_AVK>)
extern "C" int tgp_gp_loglik_grad_any(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n, const double *alpha,
                                      double *grad) {
    TGP_ARG(f && k && X && alpha && grad && n == f->n);
    if (loglik_grad_known_kind(ctx, k, "tgp_gp_loglik_grad_any")) return -1;
    return loglik_grad_from_host(ctx, f, k, X, n, alpha, grad);
}

// K build + factorisation + solve + gradient for data that live on the device (tgp_d_gp_solve followed by the above, the
// factor going back to the context's cache instead of through a handle): one call per evaluation of a gradient-driven fit.
static int d_solve_grad(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_y, const double *d_yerr,
                        double *logdet, double *ydota, double *grad) {
    TGP_HIP(hipSetDevice(ctx->device));
    int rc = tgp_ensure_io(ctx, (size_t)n * sizeof(double));
    if (rc) return rc;
    double *d_alpha = (double *)tgp_io_buffer(ctx);
    tgp_factor *f = nullptr;
    rc = tgp_d_gp_solve(ctx, k, d_X, n, d_y, d_yerr, d_alpha, logdet, ydota, &f);
    if (rc) return rc;                                      // > 0: not positive definite, nothing was kept
    rc = launch_loglik_grad(ctx, f, k, d_X, d_alpha, grad);
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]) == hipSuccess) ctx->timings[3] = ms;
    tgp_factor_release_to_cache(ctx, f);
    return rc;
}

extern "C" int tgp_d_gp_solve_grad(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_y,
                                   const double *d_yerr, double *logdet, double *ydota, double *grad) {
    TGP_ARG(k && d_X && d_y && grad && n > 0);
    if (loglik_grad_kind_check(ctx, k)) return -1;
    return d_solve_grad(ctx, k, d_X, n, d_y, d_yerr, logdet, ydota, grad);
}

// S2h: the same for every kind
extern "C" int tgp_d_gp_solve_grad_any(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_y,
                                       const double *d_yerr, double *logdet, double *ydota, double *grad) {
    TGP_ARG(k && d_X && d_y && grad && n > 0);
    if (loglik_grad_known_kind(ctx, k, "tgp_d_gp_solve_grad_any")) return -1;
    return d_solve_grad(ctx, k, d_X, n, d_y, d_yerr, logdet, ydota, grad);
}

// ---- S1s / S2s: the posterior and the likelihood gradient for sums of kernels ------------------------------------------------
// Covariance and variance differ from their namesakes in the cross panels alone (ksum.hip: every term evaluated in registers,
// one store per element); k(x_i, x_i) is the sum of the amplitudes.  With one term the namesake itself runs.
extern "C" int tgp_gp_predict_cov_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                                      const double *Xs, int64_t m, double *cov) {
    if (tgp_ksum_check(ctx, k, "tgp_gp_predict_cov_sum")) return -1;
    if (k->nterms == 1) return tgp_gp_predict_cov(ctx, f, &k->term[0], X, n, Xs, m, cov);
    TGP_ARG(f && X && Xs && cov && m > 0 && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CovPlan pl;
    int rc = cov_plan(ctx, f, m, true, &pl);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 2 * m * 8, hipMemcpyHostToDevice, st));
    rc = launch_cross_panels_sum(ctx, k, pl.d_Xs, m, pl.d_X, n, 0, pl.d_Bt, pl.Mp, pl.Np);
    if (rc) return rc;
    rc = launch_cross_panels_sum(ctx, k, pl.d_Xs, m, pl.d_Xs, m, 1, pl.d_C, pl.Mp, pl.Mp);
    if (rc) return rc;
    return cov_finish(ctx, f, pl, cov);
}

extern "C" int tgp_gp_predict_var_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                                      const double *Xs, int64_t m, double *var) {
    if (tgp_ksum_check(ctx, k, "tgp_gp_predict_var_sum")) return -1;
    if (k->nterms == 1) return tgp_gp_predict_var(ctx, f, &k->term[0], X, n, Xs, m, var);
    TGP_ARG(f && X && Xs && var && m > 0 && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t Mc = 0;
    int rc = var_chunk_rows(ctx, f, m, &Mc);
    if (rc) return rc;
    CovPlan pl;
    rc = cov_plan(ctx, f, m, true, &pl, Mc);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(pl.d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(pl.d_Xs, Xs, 2 * m * 8, hipMemcpyHostToDevice, st));
    return var_chunks(ctx, f, pl, Mc, tgp_ksum_amp(k), false, false, var, [&](const CovPlan &cp, int64_t r0, int64_t rows, int) {
        return launch_cross_panels_sum(ctx, k, cp.d_Xs + 2 * r0, rows, cp.d_X, n, 0, cp.d_Bt, cp.Mp, cp.Np);
    });
}

// 1/2 tr((alpha alpha^T - K^-1) dK/dp) is a sum over the terms: K^-1 is formed once from the factor, exactly as
// launch_loglik_grad forms it, and that function's pair pass and fixed-order reduction run once per term on the same -K^-1.
// Term t's partial sums and result live in a slot of their own in scratch2; grad (host) receives nterms x 4 numbers.
static int launch_loglik_grad_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *d_X, const double *d_alpha,
                                  double *grad) {
    hipStream_t st = ctx->stream;
    const int64_t n = f->n;
    CovPlan pl;
    int rc = cov_plan(ctx, f, n, false, &pl);             // m = n: d_Bt (Np x Np) <- L^-T, d_C (Np x Np) <- -K^-1
    if (rc) return rc;
    const int64_t nrb = (n + 63) / 64;
    const int64_t nparts = nrb * pl.nP;
    const size_t slot = (size_t)(nparts * 4 + 4);          // doubles per term: the partial sums, then the four results
    const size_t need = (size_t)k->nterms * slot * sizeof(double), stage = (size_t)pl.Mp * 1024 * sizeof(double);
    rc = tgp_ensure_scratch2(ctx, need > stage ? need : stage);
    if (rc) return rc;
    TGP_HIP(hipMemsetAsync(pl.d_Bt, 0, (size_t)pl.Mp * pl.Np * 8, st));
    TGP_HIP(hipMemsetAsync(pl.d_C, 0, (size_t)pl.Mp * pl.Mp * 8, st));
    ident_panels_kernel<<<(unsigned)(pl.Np / 256), 256, 0, st>>>(pl.d_Bt, pl.Mp, pl.Np);
    rc = cov_substitute(ctx, f, pl, true);
    if (rc) return rc;
    const int64_t mt = pl.Mp / TGP_TB;
    kinv_syrk_kernel<<<(unsigned)(mt * (mt + 1) / 2), 256, 0, st>>>(pl.d_C, pl.d_Bt, pl.Mp, pl.nP);
    const dim3 grid((unsigned)pl.nP, (unsigned)nrb);
    for (int t = 0; t < k->nterms; ++t) {
        double *partial = (double *)ctx->scratch2 + (size_t)t * slot;     // the substitution's staging buffer is free again
        const tgp_kernel *kt = &k->term[t];
        switch (kind_to_ke(kt->kind)) {                     // the caller has checked the kinds
            case KE_GAUSS: loglik_grad_kernel<KE_GAUSS><<<grid, 256, 0, st>>>(make_kparams(kt), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
            case KE_VK: loglik_grad_kernel<KE_VK><<<grid, 256, 0, st>>>(make_kparams(kt), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
            default: loglik_grad_kernel<KE_AVK><<<grid, 256, 0, st>>>(make_kparams(kt), d_X, d_alpha, pl.d_C, pl.Mp, n, partial); break;
        }
        loglik_grad_reduce_kernel<<<1, 256, 0, st>>>(partial, nparts, partial + nparts * 4);
    }
    TGP_HIP(hipGetLastError());
    TGP_HIP(hipEventRecord(ctx->ev[4], st));
    TGP_HIP(hipMemcpy2DAsync(grad, 4 * sizeof(double), (double *)ctx->scratch2 + nparts * 4, slot * sizeof(double), 4 * sizeof(double),
                             (size_t)k->nterms, hipMemcpyDeviceToHost, st));
    TGP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int tgp_gp_loglik_grad_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                                      const double *alpha, double *grad) {
    if (tgp_ksum_check(ctx, k, "tgp_gp_loglik_grad_sum")) return -1;
    if (k->nterms == 1) return tgp_gp_loglik_grad_any(ctx, f, &k->term[0], X, n, alpha, grad);
    TGP_ARG(f && X && alpha && grad && n == f->n);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = tgp_ensure_io(ctx, (size_t)3 * n * sizeof(double));          // coordinates and alpha: outside the scratch areas
    if (rc) return rc;
    double *d_X = (double *)tgp_io_buffer(ctx), *d_alpha = d_X + 2 * n;
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    TGP_HIP(hipMemcpyAsync(d_alpha, alpha, n * 8, hipMemcpyHostToDevice, st));
    rc = launch_loglik_grad_sum(ctx, f, k, d_X, d_alpha, grad);
    if (rc) return rc;
    float ms = 0.f;
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[4]));
    ctx->timings[3] = ms;
    return 0;
}

// ---- Fisher information of the hyper-parameters from a kept factor (seam S2j) ------------------------------------------------------
//   F[r][s] = 1/2 tr(C D_r C D_s) = 1/2 <S_r, S_s>,   C = (K + diag(yerr^2))^-1 = L^-T L^-1,   S_r = L^-1 D_r L^-T
// for the P = 4 T derivative matrices D_r = dK / d(log amp_t, a_t, b_t, c_t) of the T terms, in term order: the pair arithmetic of
// loglik_grad_block (post_tile.h) stored instead of summed.  The inverse of F is the covariance of the maximum-likelihood
// estimate; F does not depend on y.  Five steps, every array Np x Np in the 256-column panel layout of Bt:
//   1  fisher_dpanels_kernel   D_0 .. D_3 of one term, f and w evaluated once per pair, rows and columns >= n zero
//   2  cov_substitute          Y = D L^-T                        (the launches of the covariance, unchanged)
//   3  fisher_transpose_kernel Y^T = L^-1 D                      (D is symmetric), through LDS tiles
//   4  cov_substitute          S = Y^T L^-T
//   5  fisher_pairs_kernel     partial sums of S_r[i,j] S_s[i,j], i, j < n, per workgroup, for every pair of terms;
//      fisher_reduce_kernel    one workgroup per pair of terms adds them in a fixed order.  No atomics.
// P + 1 arrays: D_r is written to slot r + 1; Y_r is transposed into slot r, which the matrix before it has left, so S_r ends
// in slot r.  The factor is only read (its inverse slabs are built on first use, as for the covariance).
namespace {
#define TGP_FISHER_ROWS 32      // rows of a panel per workgroup of the derivative panels
template <int KE>
__device__ __forceinline__ void fisher_pair(const KParams &p, double xi, double yi, double xj, double yj, bool diag, bool in,
                                            const double *tab_f, const double *tab_w, double v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (!in) return;
    if (diag) { v[0] = p.amp; return; }                                  // d K_ii / d log amp = amp exactly, no slope
    const double dx = xi - xj, dy = yi - yj;
    double g;
    if constexpr (KE == KE_GAUSS) {
        g = p.amp * exp(-0.5 * quad_form(p, dx, dy));
        v[0] = g;
    } else {
        const double u = (KE == KE_VK) ? sqrt(dx * dx + dy * dy) * p.inv_ell : sqrt(quad_form(p, dx, dy));
        if (u == 0.0) { v[0] = p.amp; return; }                          // coincident points: f = 1, no slope
        v[0] = p.amp * vonkarman_unit_tab(u, tab_f);
        g = p.amp * vonkarman_slope_tab(u, tab_w);                       // exactly 0 beyond the value's cutoff
    }
    v[1] = -0.5 * g * dx * dx;
    v[2] = -g * dx * dy;
    v[3] = -0.5 * g * dy * dy;
}

// TGP_FISHER_ROWS rows x one 256-column panel per workgroup; a thread owns two neighbouring columns (one 16-byte store per
// array and row, 2 KiB contiguous per half workgroup), the two halves of the workgroup take alternate rows
template <int KE>
__global__ __launch_bounds__(256) void fisher_dpanels_kernel(KParams p, const double *__restrict__ X, int64_t n, int64_t Np,
                                                             double *__restrict__ D0, double *__restrict__ D1,
                                                             double *__restrict__ D2, double *__restrict__ D3) {
    __shared__ double tab_f[KE == KE_GAUSS ? 1 : 6 * K56_NDEG], tab_w[KE == KE_GAUSS ? 1 : 6 * K16_NDEG];
    if constexpr (KE != KE_GAUSS) {
        vonkarman_stage_table(tab_f);
        vonkarman_slope_stage_table(tab_w);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * TGP_PW + 2 * (tid & 127);
    const int64_t i0 = (int64_t)blockIdx.y * TGP_FISHER_ROWS + (tid >> 7);
    const bool in0 = j0 < n, in1 = j0 + 1 < n;
    const double xj0 = in0 ? X[2 * j0] : 0.0, yj0 = in0 ? X[2 * j0 + 1] : 0.0;
    const double xj1 = in1 ? X[2 * j0 + 2] : 0.0, yj1 = in1 ? X[2 * j0 + 3] : 0.0;
    for (int r = 0; r < TGP_FISHER_ROWS; r += 2) {
        const int64_t i = i0 + r;                                        // < Np: the grid covers Np / TGP_FISHER_ROWS row blocks
        const bool ini = i < n;
        const double xi = ini ? X[2 * i] : 0.0, yi = ini ? X[2 * i + 1] : 0.0;
        double v0[4], v1[4];
        fisher_pair<KE>(p, xi, yi, xj0, yj0, i == j0, ini && in0, tab_f, tab_w, v0);
        fisher_pair<KE>(p, xi, yi, xj1, yj1, i == j0 + 1, ini && in1, tab_f, tab_w, v1);
        const int64_t e = panel_elem(i, j0, Np);
        *(double2 *)(D0 + e) = make_double2(v0[0], v1[0]);
        *(double2 *)(D1 + e) = make_double2(v0[1], v1[1]);
        *(double2 *)(D2 + e) = make_double2(v0[2], v1[2]);
        *(double2 *)(D3 + e) = make_double2(v0[3], v1[3]);
    }
}

// out = in^T for Np x Np arrays in the panel layout: one 64 x 64 tile per workgroup through LDS (rows padded to 65 doubles), 16-byte
// loads and stores, 512 B contiguous per tile row on both sides
__global__ __launch_bounds__(256) void fisher_transpose_kernel(const double *__restrict__ in, double *__restrict__ out, int64_t Np) {
    __shared__ double tile[64][65];
    const int tid = threadIdx.x;
    const int c = 2 * (tid & 31), r0 = tid >> 5;
    const int64_t ti = blockIdx.y, tj = blockIdx.x;                      // the tile's rows ti * 64 .., columns tj * 64 .. of `in`
#pragma unroll
    for (int r = r0; r < 64; r += 8) {
        const double2 v = *(const double2 *)(in + panel_elem(ti * 64 + r, tj * 64 + c, Np));
        tile[r][c] = v.x;
        tile[r][c + 1] = v.y;
    }
    __syncthreads();
#pragma unroll
    for (int r = r0; r < 64; r += 8)                                     // row tj * 64 + r of `out`, columns ti * 64 + c, + 1
        *(double2 *)(out + panel_elem(tj * 64 + r, ti * 64 + c, Np)) = make_double2(tile[c][r], tile[c + 1][r]);
}

// Term pair q = blockIdx.z -> (tr >= ts): the 16 sums of S_{4 tr + r}[i,j] S_{4 ts + s}[i,j] over rows i0 .. i0 + 63 of panel
// blockIdx.x, i, j < n, to partial[((q * nrb + blockIdx.y) * nP + blockIdx.x) * 16 + 4 r + s].  A lane adds its products in row
// order, then the xor tree across the wave and the four waves in order.  `slot`: doubles between two arrays.
__global__ __launch_bounds__(256) void fisher_pairs_kernel(const double *__restrict__ S, int64_t slot, int64_t Np, int64_t n,
                                                           double *__restrict__ partial) {
    __shared__ double red[4][16];
    const int tid = threadIdx.x;
    int64_t tr, ts;
    tri_index(blockIdx.z, tr, ts);
    const double *A = S + 4 * tr * slot, *B = S + 4 * ts * slot;
    const int64_t j0 = (int64_t)blockIdx.x * TGP_PW + 2 * (tid & 127);
    const int64_t i0 = (int64_t)blockIdx.y * 64 + (tid >> 7);
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    if (j0 < n) {
        const bool in1 = j0 + 1 < n;
        for (int r = 0; r < 64; r += 2) {
            const int64_t i = i0 + r;
            if (i >= n) break;
            const int64_t e = panel_elem(i, j0, Np);
            double2 a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = *(const double2 *)(A + q * slot + e);
                b[q] = *(const double2 *)(B + q * slot + e);
                if (!in1) a[q].y = 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[4 * q + s] = fma(a[q].y, b[s].y, fma(a[q].x, b[s].x, acc[4 * q + s]));
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        double v = acc[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < 16)
        partial[(((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16 + tid] =
            (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// fixed-order sum of the `count` partial sums of term pair blockIdx.x (one workgroup each: the result does not depend on the
// schedule), the 16 sums to out[blockIdx.x * 16 ..]
__global__ __launch_bounds__(256) void fisher_reduce_kernel(const double *__restrict__ partial, int64_t count, double *__restrict__ out) {
    __shared__ double red[256][17];
    const int tid = threadIdx.x;
    const double *part = partial + (int64_t)blockIdx.x * count * 16;
    double acc[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0;
    for (int64_t q = tid; q < count; q += 256)
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] += part[q * 16 + s];
#pragma unroll
    for (int s = 0; s < 16; ++s) red[tid][s] = acc[s];
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step)
            for (int s = 0; s < 16; ++s) red[tid][s] += red[tid + step][s];
        __syncthreads();
    }
    if (tid < 16) out[(int64_t)blockIdx.x * 16 + tid] = red[0][tid];
}

// the checked arguments of both entries: -1 with a message naming `fn` and the field, before any device work
int fisher_check(tgp_ctx *ctx, const tgp_factor *f, const tgp_kernel *terms, int nterms, const double *X, int64_t n,
                 const double *fisher, const char *fn) {
    const std::string who = std::string(fn) + ": ";
    if (!f) { ctx->err = who + "f must not be NULL"; return -1; }
    if (!terms) { ctx->err = who + "k must not be NULL"; return -1; }
    if (!X) { ctx->err = who + "X must not be NULL"; return -1; }
    if (!fisher) { ctx->err = who + "fisher must not be NULL"; return -1; }
    if (n != f->n || n < 1) {
        ctx->err = who + "n = " + std::to_string((long long)n) + " is not the factor's n = " + std::to_string((long long)f->n);
        return -1;
    }
    for (int t = 0; t < nterms; ++t)
        if (kind_to_ke(terms[t].kind) < 0) {
            ctx->err = who + "unknown kernel kind " + std::to_string(terms[t].kind) + " in term " + std::to_string(t);
            return -1;
        }
    return 0;
}

int fisher_run(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *terms, int T, const double *X, int64_t n, double *fisher,
               const char *fn) {
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t Np = f->Np, nP = Np / TGP_PW;
    const int P = 4 * T, npairs = T * (T + 1) / 2;
    const int64_t nrb = (n + 63) / 64, nparts = nrb * nP;
    const int64_t slot = Np * Np;                                        // doubles per array
    TGP_ARG(Np <= 65535 && Np % TGP_PW == 0);
    // memory, before anything runs: the arena (coordinates, P + 1 arrays, partial sums and results) in `scratch`, the
    // substitution's staging in `scratch2` and, where the big-step substitution has to build them, the factor's inverse slabs
    const size_t arena = rup((size_t)2 * n * 8) + (size_t)(P + 1) * rup((size_t)slot * 8) + rup((size_t)npairs * nparts * 16 * 8) +
                         rup((size_t)npairs * 16 * 8);
    int step = 0;
    const bool no_big = getenv("TGP_COV_BIG") && atoi(getenv("TGP_COV_BIG")) == 0;
    const bool big = !no_big && potrs_big_step(Np, &step);
    const size_t staging = big ? (size_t)Np * 1024 * 8 : 0;
    const size_t slabs = (big && !f->d_slabs2 && !(f->d_slabs && f->slab_S == 1024))
                             ? vslab_bytes(Np, 1024) + (ctx->vslab_tt_bytes < (size_t)Np * 1024 * 8 ? (size_t)Np * 1024 * 8 : 0) : 0;
    size_t fr = 0, tot = 0;
    TGP_HIP(hipMemGetInfo(&fr, &tot));
    const double need = (double)arena + (double)staging + (double)slabs;
    const double avail = (double)fr + (double)ctx->scratch_bytes + (double)ctx->scratch2_bytes;
    if (need > avail) {
        ctx->err = std::string(fn) + ": needs " + std::to_string((unsigned long long)need) + " bytes of device memory (" +
                   std::to_string(P + 1) + " arrays of Np^2 = " + std::to_string((long long)Np) + "^2 doubles and the substitution's " +
                   "staging), " + std::to_string((unsigned long long)avail) + " are free";
        return -2;
    }
    int rc = tgp_ensure_scratch(ctx, arena);
    if (rc) return rc;
    char *base = (char *)ctx->scratch;
    size_t off = 0;
    auto take = [&](size_t b) { char *p = base + off; off += rup(b); return (double *)p; };
    double *d_X = take((size_t)2 * n * 8);
    double *d_S = take((size_t)slot * 8);                                // slot s at d_S + s * slotr
    const int64_t slotr = (int64_t)(rup((size_t)slot * 8) / 8);          // (= slot: Np^2 * 8 is a multiple of 256)
    off += (size_t)P * rup((size_t)slot * 8);
    double *d_part = take((size_t)npairs * nparts * 16 * 8);
    double *d_out = take((size_t)npairs * 16 * 8);
    TGP_HIP(hipEventRecord(ctx->ev[0], st));
    TGP_HIP(hipMemcpyAsync(d_X, X, (size_t)2 * n * 8, hipMemcpyHostToDevice, st));
    const dim3 dgrid((unsigned)nP, (unsigned)(Np / TGP_FISHER_ROWS));
    for (int t = 0; t < T; ++t) {
        double *D = d_S + (int64_t)(4 * t + 1) * slotr;
        const KParams p = make_kparams(&terms[t]);
        switch (kind_to_ke(terms[t].kind)) {                             // fisher_check has seen the kinds
            case KE_GAUSS: fisher_dpanels_kernel<KE_GAUSS><<<dgrid, 256, 0, st>>>(p, d_X, n, Np, D, D + slotr, D + 2 * slotr, D + 3 * slotr); break;
            case KE_VK: fisher_dpanels_kernel<KE_VK><<<dgrid, 256, 0, st>>>(p, d_X, n, Np, D, D + slotr, D + 2 * slotr, D + 3 * slotr); break;
            default: fisher_dpanels_kernel<KE_AVK><<<dgrid, 256, 0, st>>>(p, d_X, n, Np, D, D + slotr, D + 2 * slotr, D + 3 * slotr); break;
        }
    }
    TGP_HIP(hipGetLastError());
    CovPlan pl;
    pl.n = n; pl.m = n; pl.Np = Np; pl.Mp = Np;
    pl.nP = pl.nPm = (int)nP;
    pl.d_X = pl.d_Xs = pl.d_C = pl.d_v = pl.d_kss = nullptr;
    const dim3 tgrid((unsigned)(Np / 64), (unsigned)(Np / 64));
    for (int r = 0; r < P; ++r) {
        pl.d_Bt = d_S + (int64_t)(r + 1) * slotr;
        rc = cov_substitute(ctx, f, pl, false);                          // Y = D L^-T
        if (rc) return rc;
        fisher_transpose_kernel<<<tgrid, 256, 0, st>>>(pl.d_Bt, d_S + (int64_t)r * slotr, Np);
        pl.d_Bt = d_S + (int64_t)r * slotr;
        rc = cov_substitute(ctx, f, pl, false);                          // S = Y^T L^-T
        if (rc) return rc;
    }
    fisher_pairs_kernel<<<dim3((unsigned)nP, (unsigned)nrb, (unsigned)npairs), 256, 0, st>>>(d_S, slotr, Np, n, d_part);
    fisher_reduce_kernel<<<(unsigned)npairs, 256, 0, st>>>(d_part, nparts, d_out);
    TGP_HIP(hipGetLastError());
    TGP_HIP(hipEventRecord(ctx->ev[1], st));
    double sums[TGP_SUM_MAX * (TGP_SUM_MAX + 1) / 2 * 16];
    TGP_HIP(hipMemcpyAsync(sums, d_out, (size_t)npairs * 16 * 8, hipMemcpyDeviceToHost, st));
    TGP_HIP(hipStreamSynchronize(st));
    // F = 1/2 T from the lower triangle, mirrored: F[r][s] and F[s][r] carry the same bits
    for (int q = 0; q < npairs; ++q) {
        int64_t tr, ts;
        tri_index(q, tr, ts);
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int r = 4 * (int)tr + a, s = 4 * (int)ts + b;
                if (s > r) continue;
                const double v = 0.5 * sums[q * 16 + 4 * a + b];
                fisher[(size_t)r * P + s] = v;
                fisher[(size_t)s * P + r] = v;
            }
    }
    float ms = 0.f;
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->timings[3] = ms;                       // device compute
    return 0;
}
}  // namespace

extern "C" int tgp_gp_fisher(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n, double *fisher) {
    if (!ctx) return -1;
    if (fisher_check(ctx, f, k, 1, X, n, fisher, "tgp_gp_fisher")) return -1;
    return fisher_run(ctx, f, k, 1, X, n, fisher, "tgp_gp_fisher");
}

extern "C" int tgp_gp_fisher_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n, double *fisher) {
    if (!ctx) return -1;
    if (tgp_ksum_check(ctx, k, "tgp_gp_fisher_sum")) return -1;
    if (k->nterms == 1) return tgp_gp_fisher(ctx, f, &k->term[0], X, n, fisher);
    if (fisher_check(ctx, f, k->term, k->nterms, X, n, fisher, "tgp_gp_fisher_sum")) return -1;
    return fisher_run(ctx, f, k->term, k->nterms, X, n, fisher, "tgp_gp_fisher_sum");
}
