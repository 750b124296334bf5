// Sums of 2 .. TGP_SUM_MAX parametrised kernels (seams S1s / S2s of include/tgp.h).
// The reference evals any scikit-learn tree (treegp/kernels.py:17-59) and works with the matrices it returns on the host; here
// the three kernels that STORE kernel values get a sum-aware twin that evaluates every term in registers and stores once:
//   kbuild_slab_sum_kernel   : the packed K build (kbuild.hip: kbuild_slab_kernel -- same slabs, padding, identity rows, skip)
//   kernel_dense_sum_kernel  : the dense (n, m) kernel matrix (kbuild.hip: kernel_dense_kernel)
//   cross_panels_sum_kernel  : the cross panels of the posterior (cov.hip: cross_panels_kernel)
// Everything that only consumes kernel values is linear in the kernel and runs the single-kernel launches once per term
// (api.hip, cov.hip); sum_terms_kernel adds such per-term results in term order.
// Rounding contract: element = ((v_0 + v_1) + v_2) + v_3 with v_t the bits the single-kernel twin writes for term t.  The
// term loop is a run-time loop (registers: the largest evaluator's, not their sum) over a wave-uniform switch on the kind.
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "kbuild_tile.h"
#include "ksum_eval.h"

namespace {
// the four values lane l owns in one row of a slab, term t added to them
template <int KE>
__device__ __forceinline__ void slab_row_add(const KParams &p, double xi, double yi, const double (&xj)[2][2],
                                             const double (&yj)[2][2], const double *tab, double2 (&v)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        v[h].x = add_rounded(v[h].x, kb_value<KE>(p, xi - xj[h][0], yi - yj[h][0], tab));
        v[h].y = add_rounded(v[h].y, kb_value<KE>(p, xi - xj[h][1], yi - yj[h][1], tab));
    }
}

// kbuild_slab_kernel for a sum: one workgroup = 64 consecutive rows of one 256-wide panel, lane l owns columns 2l, 2l+1,
// 128+2l, 128+2l+1, wave w rows w, w + 4, ...  The Gaussian terms arrive pre-scaled by 0.5 log2 e (launch_kbuild_lower_sum).
__global__ __launch_bounds__(256) void kbuild_slab_sum_kernel(KSumParams ks, const double *__restrict__ X, int64_t n, int64_t Np,
                                                              const double *__restrict__ yerr, double *__restrict__ A) {
    constexpr int SR = 64;                                   // rows per workgroup
    __shared__ double vk_tab[6 * K56_NDEG];
    if (ks.any_vk) {                                         // (uniform over the launch)
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
    double xj[2][2], yj[2][2];
    int padbits = 0;                                         // bit 2 h + e: column jc[h] + e is padding
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t j = jc[h] + e;
            xj[h][e] = j < n ? X[2 * j] : 0.0;
            yj[h][e] = j < n ? X[2 * j + 1] : 0.0;
            if (j >= n) padbits |= 1 << (2 * h + e);
        }
    // The slab's uniform flags travel in ONE scalar register and are tested from it in every row: kept as booleans they are
    // hoisted out of the row loop as 64-bit lane masks, two SGPRs each, live across the term loop -- whose three evaluators'
    // fp64 literals leave none to spare (the masks spilled to VGPR lanes).
    enum { F_DIAG = 1, F_SKIP = 2, F_PAD = 4, F_YERR = 8 };
    const int slab_flags = __builtin_amdgcn_readfirstlane(
        (slab < TGP_PW / SR ? F_DIAG : 0)                     // rows inside the panel's 256 x 256 diagonal block
        | (slab < TGP_TB / SR ? F_SKIP : 0)                   // first 128 rows: the second tile lies above the diagonal
        | ((i0 + SR > n) || (pj * TGP_PW + TGP_PW > n) ? F_PAD : 0) | (yerr ? F_YERR : 0) | (ks.nterms << 4));   // and the term count

    for (int r = wave; r < SR; r += 4) {
        const int64_t i = i0 + r;
        double2 v[2];
        int fl = slab_flags;
        asm volatile("" : "+s"(fl));
        const bool diag_slab = fl & F_DIAG, upper_half_skip = fl & F_SKIP, pad_slab = fl & F_PAD;
        if (!pad_slab || i < n) {
            const int64_t ic = i < n ? i : 0;
            const double xi = X[2 * ic], yi = X[2 * ic + 1];                       // wave-uniform
            v[0].x = v[0].y = v[1].x = v[1].y = -0.0;                              // -0 + v_0 is v_0, bit for bit
            int t = 0;                                                             // (nterms >= 2: the launcher's one-term case
#pragma unroll 1                                                                   //  is the single-kernel build)
            do {
                switch (ks.ke[t]) {                                                // launch-uniform
                    case KE_GAUSS: slab_row_add<KE_GAUSS>(ks.t[t], xi, yi, xj, yj, vk_tab, v); break;
                    case KE_VK: slab_row_add<KE_VK>(ks.t[t], xi, yi, xj, yj, vk_tab, v); break;
                    default: slab_row_add<KE_AVK>(ks.t[t], xi, yi, xj, yj, vk_tab, v); break;
                }
            } while (++t < (fl >> 4));
            if (diag_slab) {
                // exact diagonal (kernels.py:121, summed over the terms) + noise (gp_interp.py:180)
                const double e = (fl & F_YERR) ? yerr[ic] : 0.0;
                const double d = ks.ampsum + e * e;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (i == jc[h]) v[h].x = d;
                    if (i == jc[h] + 1) v[h].y = d;
                }
            }
            if (pad_slab) {
                // the flags are tested from one VGPR per row: as four comparisons against n they would be hoisted out of the row
                // loop as four lane masks, eight SGPRs live across the term loop, which has none to spare (they spilled)
                int pb = padbits;
                asm volatile("" : "+v"(pb));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (pb & (1 << (2 * h))) v[h].x = 0.0;
                    if (pb & (2 << (2 * h))) v[h].y = 0.0;
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
        kb_store(dst + (int64_t)r * TGP_PW, v[0]);
        if (!upper_half_skip) kb_store(dst + (int64_t)r * TGP_PW + TGP_TB, v[1]);
    }
}

// sum over the terms of kernel_value<KE>: what kernel_dense_kernel and cross_panels_kernel evaluate, term by term
__device__ __forceinline__ double sum_value(const KSumParams &ks, double dx, double dy) {
    double v = -0.0;
#pragma unroll 1
    for (int t = 0; t < ks.nterms; ++t) {
        double vt;
        switch (ks.ke[t]) {
            case KE_GAUSS: vt = kernel_value<KE_GAUSS>(ks.t[t], dx, dy); break;
            case KE_VK: vt = kernel_value<KE_VK>(ks.t[t], dx, dy); break;
            default: vt = kernel_value<KE_AVK>(ks.t[t], dx, dy); break;
        }
        v = add_rounded(v, vt);
    }
    return v;
}

// dense out[i*m + j] = sum_t amp_t k_t(X_i, Y_j); self != 0: Y == X and the diagonal is exactly the sum of the amplitudes
__global__ __launch_bounds__(256) void kernel_dense_sum_kernel(KSumParams ks, const double *__restrict__ X, int64_t n,
                                                               const double *__restrict__ Y, int64_t m, int self,
                                                               double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * 16;
    if (j >= m) return;
    const double xj = Y[2 * j], yj = Y[2 * j + 1];
    for (int r = 0; r < 16; ++r) {
        const int64_t i = i0 + r;
        if (i >= n) break;
        double v = sum_value(ks, X[2 * i] - xj, X[2 * i + 1] - yj);
        if (self && i == j) v = ks.ampsum;
        out[i * m + j] = v;
    }
}

// out: panels of 256 columns, panel p at out + p * rows * 256, element (i, j) -> [i][j & 255]; 0 outside (m, n)
__global__ __launch_bounds__(256) void cross_panels_sum_kernel(KSumParams ks, const double *__restrict__ Xs, int64_t m,
                                                               const double *__restrict__ X, int64_t n, int self,
                                                               double *__restrict__ out, int64_t rows, int64_t ncols) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= ncols) return;
    double v = 0.0;
    if (i < m && j < n) {
        v = sum_value(ks, Xs[2 * i] - X[2 * j], Xs[2 * i + 1] - X[2 * j + 1]);
        if (self && i == j) v = ks.ampsum;
    }
    out[(j >> 8) * rows * TGP_PW + i * TGP_PW + (j & 255)] = v;
}

// out[i] = ((T[0][i] + T[1][i]) + ...) over `nterms` arrays of `stride` doubles: per-term results added in term order
__global__ __launch_bounds__(256) void sum_terms_kernel(const double *__restrict__ T, int nterms, int64_t stride, int64_t count,
                                                        double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double v = T[i];
    for (int t = 1; t < nterms; ++t) v += T[(int64_t)t * stride + i];
    out[i] = v;
}

}  // namespace

double tgp_ksum_amp(const tgp_kernel_sum *k) {
    volatile double s = k->term[0].amp;                      // (volatile: one rounding per add, whatever the host compiler does)
    for (int t = 1; t < k->nterms; ++t) s = s + k->term[t].amp;
    return s;
}

int tgp_ksum_check(tgp_ctx *ctx, const tgp_kernel_sum *k, const char *fn) {
    if (!k) {
        ctx->err = std::string(fn) + ": null kernel sum";
        return -1;
    }
    if (k->nterms < 1 || k->nterms > TGP_SUM_MAX) {
        ctx->err = std::string(fn) + ": nterms = " + std::to_string(k->nterms) + " outside 1 .. " + std::to_string(TGP_SUM_MAX);
        return -1;
    }
    for (int t = 0; t < k->nterms; ++t)
        if (kind_to_ke(k->term[t].kind) < 0) {
            ctx->err = std::string(fn) + ": unknown kernel kind " + std::to_string(k->term[t].kind) + " in term " + std::to_string(t);
            return -1;
        }
    return 0;
}

// Two or more terms always take the slab kernel: launch_kbuild_lower's A/B switch TGP_KBUILD_TILES (the first-generation
// 128 x 128 tile kernel, which evaluates with other bits and writes other elements above the diagonal) does not apply to sums.
int launch_kbuild_lower_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *d_X, int64_t n, int64_t Np,
                            const double *d_yerr, double *d_A) {
    if (k->nterms == 1) return launch_kbuild_lower(ctx, &k->term[0], d_X, n, Np, d_yerr, d_A);
    const KSumParams ks = make_ksum(k, true);
    const int64_t P = Np / TGP_PW;
    kbuild_slab_sum_kernel<<<(unsigned)(4 * (P * (P + 1) / 2)), 256, 0, ctx->stream>>>(ks, d_X, n, Np, d_yerr, d_A);
    TGP_HIP(hipGetLastError());
    return 0;
}

int launch_kernel_dense_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *d_X, int64_t n, const double *d_Y,
                            int64_t m, int self, double *d_out) {
    if (k->nterms == 1) return launch_kernel_dense(ctx, &k->term[0], d_X, n, d_Y, m, self, d_out);
    const KSumParams ks = make_ksum(k, false);
    dim3 grid((unsigned)((m + 255) / 256), (unsigned)((n + 15) / 16)), block(256);
    kernel_dense_sum_kernel<<<grid, block, 0, ctx->stream>>>(ks, d_X, n, d_Y, m, self, d_out);
    TGP_HIP(hipGetLastError());
    return 0;
}

int launch_cross_panels_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *d_Xs, int64_t m, const double *d_X, int64_t n,
                            int self, double *d_out, int64_t rows, int64_t ncols) {
    TGP_ARG(rows <= 65535);
    const KSumParams ks = make_ksum(k, false);
    dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)rows), block(256);
    cross_panels_sum_kernel<<<grid, block, 0, ctx->stream>>>(ks, d_Xs, m, d_X, n, self, d_out, rows, ncols);
    TGP_HIP(hipGetLastError());
    return 0;
}

int launch_sum_terms(tgp_ctx *ctx, const double *d_T, int nterms, int64_t stride, int64_t count, double *d_out) {
    sum_terms_kernel<<<(unsigned)((count + 255) / 256), 256, 0, ctx->stream>>>(d_T, nterms, stride, count, d_out);
    TGP_HIP(hipGetLastError());
    return 0;
}

extern "C" int tgp_d_kbuild_lower_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *d_X, int64_t n, const double *d_yerr,
                                      double *d_A) {
    if (tgp_ksum_check(ctx, k, "tgp_d_kbuild_lower_sum")) return -1;
    if (k->nterms == 1) return tgp_d_kbuild_lower(ctx, &k->term[0], d_X, n, d_yerr, d_A);
    TGP_ARG(d_X && d_A && n > 0);
    TGP_HIP(hipSetDevice(ctx->device));
    const int64_t Np = padded_n(n);
    TGP_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    int rc = launch_kbuild_lower_sum(ctx, k, d_X, n, Np, d_yerr, d_A);
    if (rc) return rc;
    TGP_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    TGP_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->timings[0] = ms;
    ctx->timings[8] = 8.0 * ((double)Np * (Np + 1) / 2.0) + 16.0 * (double)Np;
    return 0;
}

extern "C" int tgp_kernel_matrix_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *X, int64_t n, const double *Y, int64_t m,
                                     double *out) {
    if (tgp_ksum_check(ctx, k, "tgp_kernel_matrix_sum")) return -1;
    if (k->nterms == 1) return tgp_kernel_matrix(ctx, &k->term[0], X, n, Y, m, out);
    TGP_ARG(X && out && n > 0);
    const int self = (Y == nullptr);
    if (self) m = n;
    TGP_ARG(m > 0);
    TGP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = tgp_ensure_io(ctx, rup(2 * n * 8) + rup(2 * m * 8) + rup((size_t)n * m * 8));
    if (rc) return rc;
    char *base = (char *)tgp_io_buffer(ctx);
    double *d_X = (double *)base, *d_Y = (double *)(base + rup(2 * n * 8)), *d_o = (double *)(base + rup(2 * n * 8) + rup(2 * m * 8));
    TGP_HIP(hipMemcpyAsync(d_X, X, 2 * n * 8, hipMemcpyHostToDevice, st));
    if (!self) TGP_HIP(hipMemcpyAsync(d_Y, Y, 2 * m * 8, hipMemcpyHostToDevice, st));
    rc = launch_kernel_dense_sum(ctx, k, d_X, n, self ? d_X : d_Y, m, self, d_o);
    if (rc) return rc;
    TGP_HIP(hipMemcpyAsync(out, d_o, (size_t)n * m * 8, hipMemcpyDeviceToHost, st));
    TGP_HIP(hipStreamSynchronize(st));
    return 0;
}
