// Many small GPs in one launch sequence (seam S2e of include/tgp.h; replaces the reference's one cholesky + cho_solve per
// GP, treegp/gp_interp.py:180-182, and per likelihood evaluation, treegp/log_likelihood.py:29-33, 43-62).
//
// Every problem of a chunk is stored like a single solve at the chunk's common Np (packed panels): problem b's
// panels at b * tgp_panel_elems(Np), its inverted diagonal blocks at b * Np * 128; rows >= n_b carry the identity.  Every
// launch covers all problems of the chunk, the problem index being the grid's y dimension, and runs the existing device
// bodies through thin wrappers that only offset pointers by it:
//   K build        kbuild_tile (kbuild_tile.h), once per kernel evaluator present
//   per panel k    potrf128_body (0,0) -> rows below: X = A W0^T -> A[:,128:] -= X L10^T -> potrf128_body (1,1) ->
//                  rows below: X = A W1^T (gemm_tile_128) -> trailing update, depth 256 (gemm_tile_dtv)
//   sweeps         one launch per 128-block and direction: the block's GEMV with W = L_jj^-1 and the update of the other blocks
//   logdet, chi2   one workgroup per problem
// Plain launches on the context's one stream, no in-kernel waits, no atomics in any sum.  Tile forms and summation depths
// depend only on the panel index and Np, so a problem's bits do not depend on its companions, its place or the chunking.
#define TGP_POTRF_BODY_ONLY
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "kbuild_tile.h"
#include "gemm_tile.h"
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
    y[d] = in ? ry[s] : 0.0;
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

// ---- K + diag(yerr^2): one 128 x 128 tile per workgroup, blockIdx.y = the y-th problem of this evaluator ---------------------
template <int KE>
__global__ __launch_bounds__(256) void bkbuild_kernel(const KParams *__restrict__ kp, const int *__restrict__ list,
                                                      const int64_t *__restrict__ ns, const double *__restrict__ X,
                                                      const double *__restrict__ e, BatchDims d, double *__restrict__ A) {
    const int b = list[blockIdx.y];
    const int64_t t = blockIdx.x;
    int64_t ti = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int64_t tj = t - ti * (ti + 1) / 2;
    const int64_t pj = tj >> 1;
    double *tile = A + b * d.ae + panel_off(pj, d.Np) + (ti * TGP_TB - pj * TGP_PW) * TGP_PW + (tj & 1) * TGP_TB;
    const KParams p = kp[b];
    kbuild_tile<KE>(p, X + (int64_t)b * 2 * d.Np, ns[b], e ? e + (int64_t)b * d.Np : nullptr, ti, tj, tile);
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
    const int64_t t = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)ti * (ti + 1) / 2 > t) --ti;
    while ((int64_t)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = (int)(t - (int64_t)ti * (ti + 1) / 2);
    double *Ab = A + blockIdx.y * d.ae;
    const double *P = Ab + panel_off(k, d.Np) + (int64_t)TGP_PW * TGP_PW;      // panel k from row 256 (k + 1)
    const int ob = k + 1;
    const int64_t pj = ob + (tj >> 1);
    const int64_t I = (int64_t)TGP_PW * ob + (int64_t)TGP_TB * ti;
    double *C = Ab + panel_off(pj, d.Np) + (I - pj * TGP_PW) * TGP_PW + (tj & 1) * TGP_TB;
    gemm_tile_dtv<4, TGP_PW, 1>(P + (int64_t)ti * TGP_TB * TGP_PW, P + (int64_t)tj * TGP_TB * TGP_PW, C, nullptr, nullptr);
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

inline size_t rup(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// problems per chunk: TGP_BATCH_CHUNK, or as many as 90 % of the free device memory holds (the context's own scratch counted as
// free: it is given back before a bigger one is taken)
static int64_t batch_chunk(tgp_ctx *ctx, int nb, size_t per, size_t fixed, int *rc) {
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
        ctx->err = "tgp_gp_solve_batch: not enough free device memory for one problem of this order";
        *rc = -2;
    }
    return c;
}

int tgp_gp_solve_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                       const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info) {
    if (!ctx) return -1;
    if (nb < 1) { ctx->err = "tgp_gp_solve_batch: nb must be >= 1"; return -1; }
    if (nmax < 1 || nmax > 4096) { ctx->err = "tgp_gp_solve_batch: nmax must be in 1 .. 4096 (larger problems: tgp_gp_solve)"; return -1; }
    TGP_ARG(ks && ns && X && y && logdet && info);
    for (int b = 0; b < nb; ++b) {
        if (ns[b] < 1 || ns[b] > nmax) {
            ctx->err = "tgp_gp_solve_batch: ns[" + std::to_string(b) + "] = " + std::to_string((long long)ns[b]) + " is not in 1 .. nmax = " +
                       std::to_string((long long)nmax);
            return -1;
        }
        if (kind_to_ke(ks[b].kind) < 0) {
            ctx->err = "tgp_gp_solve_batch: ks[" + std::to_string(b) + "].kind = " + std::to_string(ks[b].kind) + " is not a kernel kind";
            return -1;
        }
    }
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t Np = padded_n(nmax), nP = Np / TGP_PW, nT = Np / TGP_TB;
    const BatchDims d{Np, panel_off(nP, Np), Np * TGP_TB};
    const size_t per = rup((size_t)d.ae * 8) + rup((size_t)d.we * 8) + 6 * rup((size_t)Np * 8) + 5 * rup((size_t)nmax * 8) +
                       rup(sizeof(KParams)) + 2 * rup(8) + 2 * rup(16);
    const size_t fixed = 8 * 256;
    int rc = 0;
    const int64_t C = batch_chunk(ctx, nb, per, fixed, &rc);
    if (rc) return rc;
    // one arena per chunk size: arrays of C problems each
    const size_t need = (size_t)C * per + fixed;
    rc = tgp_ensure_scratch(ctx, need);
    if (rc) return rc;
    char *base = (char *)ctx->scratch;
    size_t off = 0;
    auto take = [&](size_t bytes) { void *p = base + off; off += rup(bytes); return p; };
    double *dA = (double *)take((size_t)C * d.ae * 8);
    double *dW = (double *)take((size_t)C * d.we * 8);
    double *dX = (double *)take((size_t)C * 2 * Np * 8);
    double *dy = (double *)take((size_t)C * Np * 8);
    double *de = (double *)take((size_t)C * Np * 8);
    double *dz = (double *)take((size_t)C * Np * 8);
    double *da = (double *)take((size_t)C * Np * 8);
    double *rX = (double *)take((size_t)C * 2 * nmax * 8);
    double *ry = (double *)take((size_t)C * nmax * 8);
    double *re = (double *)take((size_t)C * nmax * 8);
    double *ra = (double *)take((size_t)C * nmax * 8);
    KParams *dkp = (KParams *)take((size_t)C * sizeof(KParams));
    int64_t *dns = (int64_t *)take((size_t)C * 8);
    int *dlist = (int *)take((size_t)C * 4);
    int *dinfo = (int *)take((size_t)C * 4);
    double *dout = (double *)take((size_t)C * 16);
    // host side of the small tables and results: the context's pinned scratch
    const size_t hbytes = rup((size_t)C * sizeof(KParams)) + rup((size_t)C * 8) + rup((size_t)C * 4) + rup((size_t)C * 4) + rup((size_t)C * 16);
    void *hp = nullptr;
    rc = tgp_ensure_pinned(ctx, hbytes, &hp);
    if (rc) return rc;
    char *hb = (char *)hp;
    KParams *hkp = (KParams *)hb;
    int64_t *hns = (int64_t *)(hb + rup((size_t)C * sizeof(KParams)));
    int *hlist = (int *)((char *)hns + rup((size_t)C * 8));
    int *hinfo = (int *)((char *)hlist + rup((size_t)C * 4));
    double *hout = (double *)((char *)hinfo + rup((size_t)C * 4));

    static bool attr_ok = hipFuncSetAttribute((const void *)bpotrf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)potrf_v2::POTRF_LDS_BYTES) == hipSuccess;
    if (!attr_ok) { ctx->err = "tgp_gp_solve_batch: the diagonal-block kernel cannot have its LDS image"; return -2; }

    double ms_k = 0.0, ms_c = 0.0, ms_s = 0.0;
    for (int64_t c0 = 0; c0 < nb; c0 += C) {
        const int64_t cn = (nb - c0) < C ? (nb - c0) : C;
        // evaluator lists: the problems of this chunk grouped by kernel evaluator, each group in batch order
        int cnt[3] = {0, 0, 0};
        for (int64_t b = 0; b < cn; ++b) {
            hkp[b] = make_kparams(&ks[c0 + b]);
            hns[b] = ns[c0 + b];
            ++cnt[kind_to_ke(ks[c0 + b].kind)];
        }
        int start[3] = {0, cnt[0], cnt[0] + cnt[1]}, fill[3] = {0, 0, 0};
        for (int64_t b = 0; b < cn; ++b) {
            const int k = kind_to_ke(ks[c0 + b].kind);
            hlist[start[k] + fill[k]++] = (int)b;
        }
        TGP_HIP(hipMemcpyAsync(dkp, hkp, (size_t)cn * sizeof(KParams), hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(dns, hns, (size_t)cn * 8, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(dlist, hlist, (size_t)cn * 4, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(rX, X + c0 * nmax * 2, (size_t)cn * nmax * 16, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(ry, y + c0 * nmax, (size_t)cn * nmax * 8, hipMemcpyHostToDevice, st));
        if (yerr) TGP_HIP(hipMemcpyAsync(re, yerr + c0 * nmax, (size_t)cn * nmax * 8, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemsetAsync(dinfo, 0, (size_t)cn * 4, st));
        const unsigned ncn = (unsigned)cn;
        bpad_kernel<<<dim3((unsigned)(Np / 256), ncn), 256, 0, st>>>(rX, ry, yerr ? re : nullptr, dns, nmax, Np, dX, dy,
                                                                     yerr ? de : nullptr);
        const double *e_or_null = yerr ? de : nullptr;

        TGP_HIP(hipEventRecord(ctx->ev[0], st));
        const unsigned ntiles = (unsigned)(nT * (nT + 1) / 2);
        if (cnt[0]) bkbuild_kernel<KE_GAUSS><<<dim3(ntiles, cnt[0]), 256, 0, st>>>(dkp, dlist + start[0], dns, dX, e_or_null, d, dA);
        if (cnt[1]) bkbuild_kernel<KE_VK><<<dim3(ntiles, cnt[1]), 256, 0, st>>>(dkp, dlist + start[1], dns, dX, e_or_null, d, dA);
        if (cnt[2]) bkbuild_kernel<KE_AVK><<<dim3(ntiles, cnt[2]), 256, 0, st>>>(dkp, dlist + start[2], dns, dX, e_or_null, d, dA);
        TGP_HIP(hipEventRecord(ctx->ev[1], st));

        // right-looking, one 256-wide panel at a time
        for (int k = 0; k < (int)nP; ++k) {
            const int64_t pk = panel_off(k, Np), mk = Np - (int64_t)TGP_PW * k;
            const int64_t w0 = (int64_t)(2 * k) * TGP_TB * TGP_TB, w1 = w0 + TGP_TB * TGP_TB;
            const int64_t r1 = pk + (int64_t)TGP_TB * TGP_PW;          // row 128 of the panel
            const unsigned nr1 = (unsigned)((mk - TGP_TB) / TGP_TB), nr2 = (unsigned)((mk - TGP_PW) / TGP_TB);
            bpotrf_kernel<<<ncn, 256, potrf_v2::POTRF_LDS_BYTES, st>>>(dA, dW, d, pk, w0, dinfo, k * TGP_PW);
            bgemm_col_kernel<0, TGP_TB, true><<<dim3(nr1, ncn), 256, 0, st>>>(dA, dW, d, r1, w0, r1);
            bgemm_col_kernel<1, TGP_PW, false><<<dim3(nr1, ncn), 256, 0, st>>>(dA, dW, d, r1, r1, r1 + TGP_TB);
            bpotrf_kernel<<<ncn, 256, potrf_v2::POTRF_LDS_BYTES, st>>>(dA, dW, d, r1 + TGP_TB, w1, dinfo, k * TGP_PW + TGP_TB);
            if (nr2 == 0) continue;
            const int64_t r2 = pk + (int64_t)TGP_PW * TGP_PW + TGP_TB;   // row 256, column 128
            bgemm_col_kernel<0, TGP_TB, true><<<dim3(nr2, ncn), 256, 0, st>>>(dA, dW, d, r2, w1, r2);
            bsyrk_kernel<<<dim3((unsigned)(nr2 * (nr2 + 1) / 2), ncn), 256, 0, st>>>(dA, d, k, (int)nr2);
        }
        TGP_HIP(hipEventRecord(ctx->ev[2], st));

        for (int j = 0; j < (int)nT; ++j)
            bfwd_step_kernel<<<dim3((unsigned)(nT - j), ncn), 256, 0, st>>>(dA, dW, d, dy, dz, j);
        bfinish_kernel<<<ncn, 256, 0, st>>>(dA, dz, dns, d, dout);
        if (alpha) {
            for (int j = (int)nT - 1; j >= 0; --j)
                bbwd_step_kernel<<<dim3((unsigned)(j + 1), ncn), 256, 0, st>>>(dA, dW, d, dz, da, j);
            bunpad_kernel<<<dim3((unsigned)((nmax + 255) / 256), ncn), 256, 0, st>>>(da, dns, nmax, Np, ra);
        }
        TGP_HIP(hipEventRecord(ctx->ev[3], st));
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipMemcpyAsync(hinfo, dinfo, (size_t)cn * 4, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipMemcpyAsync(hout, dout, (size_t)cn * 16, hipMemcpyDeviceToHost, st));
        if (alpha) TGP_HIP(hipMemcpyAsync(alpha + c0 * nmax, ra, (size_t)cn * nmax * 8, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipStreamSynchronize(st));
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        TGP_HIP(hipEventElapsedTime(&t0, ctx->ev[0], ctx->ev[1]));
        TGP_HIP(hipEventElapsedTime(&t1, ctx->ev[1], ctx->ev[2]));
        TGP_HIP(hipEventElapsedTime(&t2, ctx->ev[2], ctx->ev[3]));
        ms_k += t0;
        ms_c += t1;
        ms_s += t2;
        for (int64_t b = 0; b < cn; ++b) {
            if (hinfo[b] < 0) {
                ctx->err = "tgp_gp_solve_batch: a diagonal block of problem " + std::to_string((long long)(c0 + b)) +
                           " reported an internal hand-off failure (info " + std::to_string(hinfo[b]) + ")";
                return -2;
            }
            info[c0 + b] = hinfo[b];
            logdet[c0 + b] = hout[2 * b];
            if (ydota) ydota[c0 + b] = hout[2 * b + 1];
        }
    }
    // only the slots this call fills: nothing of an earlier call on the context is left behind in the others
    for (int i = 0; i < TGP_NTIMINGS; ++i) ctx->timings[i] = 0.0;
    ctx->timings[0] = ms_k;
    ctx->timings[1] = ms_c;
    ctx->timings[2] = ms_s;
    ctx->timings[10] = alpha ? 2.0 : 1.0;
    return 0;
}
