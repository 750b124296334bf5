// Sums of 1 .. TGP_SUM_MAX parametrised kernels on the device: the parameter block and the rounding contract shared by ksum.hip
// (one problem per launch, seams S1s / S2s of include/tgp.h) and batch.hip (the problem index on the grid, seam S2i).
// An element is ((v_0 + v_1) + v_2) + v_3, plain fp64 adds in term order, v_t the bits the single-kernel twin writes for term t.
#pragma once
#include "tgp_internal.h"
#include "kernel_eval.h"

struct KSumParams {
    KParams t[TGP_SUM_MAX];
    int ke[TGP_SUM_MAX];
    double ampsum;            // ((amp_0 + amp_1) + ...): the exact diagonal of a self matrix
    int nterms;
    int any_vk;
};

// acc + v with v already rounded: the compiler must neither see the amplitude multiply behind v (it would contract
// amp * k + acc into one FMA, and the element would no longer be the sum of the single-kernel values) nor fuse the add
__device__ __forceinline__ double add_rounded(double acc, double v) {
    asm volatile("" : "+v"(v));
    return __dadd_rn(acc, v);
}

// `nterms` terms read through `term(t)`; slab_scaling: the Gaussian terms pre-scaled by 0.5 log2 e, as launch_kbuild_lower
template <class Term>
static inline KSumParams make_ksum_terms(int nterms, Term term, bool slab_scaling) {
    KSumParams ks;
    memset(&ks, 0, sizeof(ks));
    ks.nterms = nterms;
    volatile double s = 0.0;                                 // (volatile: one rounding per add, as tgp_ksum_amp)
    for (int t = 0; t < nterms; ++t) {
        const tgp_kernel *k = term(t);
        ks.t[t] = make_kparams(k);
        ks.ke[t] = kind_to_ke(k->kind);
        if (ks.ke[t] != KE_GAUSS) ks.any_vk = 1;
        if (slab_scaling && ks.ke[t] == KE_GAUSS) {
            const double c0 = 0.72134752044448170368;                        // 0.5 log2 e, as launch_kbuild_lower
            ks.t[t].a *= c0;
            ks.t[t].b2 *= c0;
            ks.t[t].c *= c0;
        }
        s = t ? s + k->amp : k->amp;
    }
    ks.ampsum = s;
    return ks;
}

static inline KSumParams make_ksum(const tgp_kernel_sum *k, bool slab_scaling) {
    return make_ksum_terms(k->nterms, [k](int t) { return &k->term[t]; }, slab_scaling);
}

// sum over the terms of kernel_value<KE>, term by term.  ANYVK = false: every term is Gaussian and the instantiation carries
// no Bessel evaluator (60 VGPRs against 166: the lesson above bloglik_grad_kernel of batch.hip); `ks.ke` is then not read.
// The term loop is a run-time loop (registers: the largest evaluator's, not their sum) over a wave-uniform switch on the kind.
template <bool ANYVK>
__device__ __forceinline__ double ksum_value(const KSumParams &ks, double dx, double dy) {
    double v = -0.0;                                         // -0 + v_0 is v_0, bit for bit
    int t = 0;
#pragma unroll 1
    do {
        double vt;
        if constexpr (!ANYVK) {
            vt = kernel_value<KE_GAUSS>(ks.t[t], dx, dy);
        } else {
            switch (ks.ke[t]) {
                case KE_GAUSS: vt = kernel_value<KE_GAUSS>(ks.t[t], dx, dy); break;
                case KE_VK: vt = kernel_value<KE_VK>(ks.t[t], dx, dy); break;
                default: vt = kernel_value<KE_AVK>(ks.t[t], dx, dy); break;
            }
        }
        v = add_rounded(v, vt);
    } while (++t < ks.nterms);
    return v;
}

// the two values a lane owns in one row of a tile: ksum_value for both under one term loop and one switch
template <int KE>
__device__ __forceinline__ void ksum_add2(const KParams &p, double dx0, double dy0, double dx1, double dy1, double2 &v) {
    v.x = add_rounded(v.x, kernel_value<KE>(p, dx0, dy0));
    v.y = add_rounded(v.y, kernel_value<KE>(p, dx1, dy1));
}
template <bool ANYVK>
__device__ __forceinline__ void ksum_value2(const KSumParams &ks, double dx0, double dy0, double dx1, double dy1, double2 &v) {
    v.x = v.y = -0.0;
    int t = 0;
#pragma unroll 1
    do {
        if constexpr (!ANYVK) {
            ksum_add2<KE_GAUSS>(ks.t[t], dx0, dy0, dx1, dy1, v);
        } else {
            switch (ks.ke[t]) {
                case KE_GAUSS: ksum_add2<KE_GAUSS>(ks.t[t], dx0, dy0, dx1, dy1, v); break;
                case KE_VK: ksum_add2<KE_VK>(ks.t[t], dx0, dy0, dx1, dy1, v); break;
                default: ksum_add2<KE_AVK>(ks.t[t], dx0, dy0, dx1, dy1, v); break;
            }
        }
    } while (++t < ks.nterms);
}

// kbuild_tile (kbuild_tile.h) for a sum: the same 128 x 128 tile, lane ownership, padding, identity rows and store pattern; every
// term evaluated in registers, the tile stored once.  The diagonal is ampsum + yerr_i^2.
template <bool ANYVK>
__device__ __forceinline__ void kbuild_tile_sum(const KSumParams &ks, const double *__restrict__ X, int64_t n,
                                                const double *__restrict__ yerr, int64_t ti, int64_t tj,
                                                double *__restrict__ tile) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j0 = tj * TGP_TB + 2 * lane;
    double xj0 = 0, yj0 = 0, xj1 = 0, yj1 = 0;
    if (j0 < n) { xj0 = X[2 * j0]; yj0 = X[2 * j0 + 1]; }
    if (j0 + 1 < n) { xj1 = X[2 * j0 + 2]; yj1 = X[2 * j0 + 3]; }

    const bool diag_tile = (ti == tj);
    const bool pad_tile = (ti * TGP_TB + TGP_TB > n);   // rows (and maybe columns) beyond n

    for (int r = wave; r < TGP_TB; r += 4) {
        const int64_t i = ti * TGP_TB + r;
        double2 v;
        if (!pad_tile || i < n) {
            const double xi = X[2 * (i < n ? i : 0)], yi = X[2 * (i < n ? i : 0) + 1];   // wave-uniform
            ksum_value2<ANYVK>(ks, xi - xj0, yi - yj0, xi - xj1, yi - yj1, v);
            if (diag_tile) {
                // exact diagonal (kernels.py:121, summed over the terms) + noise (gp_interp.py:180)
                if (i == j0) { const double e = yerr ? yerr[i] : 0.0; v.x = ks.ampsum + e * e; }
                if (i == j0 + 1) { const double e = yerr ? yerr[i] : 0.0; v.y = ks.ampsum + e * e; }
            }
            if (pad_tile) {
                if (j0 >= n) v.x = 0.0;
                if (j0 + 1 >= n) v.y = 0.0;
            }
        } else {
            // padded rows: identity, so the padded factor is [[L, 0], [0, I]]
            v.x = (i == j0) ? 1.0 : 0.0;
            v.y = (i == j0 + 1) ? 1.0 : 0.0;
        }
        *reinterpret_cast<double2 *>(tile + (int64_t)r * TGP_PW + 2 * lane) = v;
    }
}

// cross_value<KE> (post_tile.h) summed over the terms: 0 outside (m, n); `self`: x is xs and the diagonal is exactly ampsum
template <bool ANYVK>
__device__ __forceinline__ double cross_value_sum(const KSumParams &ks, const double *__restrict__ xs, int64_t m,
                                                  const double *__restrict__ x, int64_t n, int self, int64_t i, int64_t j) {
    double v = 0.0;
    if (i < m && j < n) {
        v = ksum_value<ANYVK>(ks, xs[2 * i] - x[2 * j], xs[2 * i + 1] - x[2 * j + 1]);
        if (self && i == j) v = ks.ampsum;
    }
    return v;
}
