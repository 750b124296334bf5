/* tgp.h -- C-ABI of libtgp.so: the MI355X-native GP hot path behind treegp's Python API.
 *
 * The reference (PFLeget/treegp, pure Python) has no FFI of its own; it calls SciPy /
 * scikit-learn / TreeCorr at a handful of seams.  Each entry point below replaces one of those
 * seams and cites the reference lines it stands in for (paths relative to the reference root).
 *
 *   S1  kernel.__call__(X[,Y])           treegp/kernels.py:114-126, 249-276, 355-381
 *   S2  cholesky + cho_solve (+ logdet)  treegp/gp_interp.py:180-182, treegp/log_likelihood.py:29-33
 *   S2e many small S2 at once           treegp/gp_interp.py:180-182, treegp/log_likelihood.py:29-33, 43-62, README.rst:28
 *   S2f many small S2 + S2d at once     treegp/log_likelihood.py:43-62 for the problems of S2e (one evaluation of many fits)
 *   S2g many small S2 + diag(K^-1)      not in the reference: leave-one-out for the problems of S2e (R&W 5.4.2)
 *   S1s / S2s  S1, S2, S3 .. S3c for sums of kernels   treegp/kernels.py:17-59 (eval_kernel evals any tree)
 *   S2j Fisher information of the hyper-parameters   not in the reference: error bars on a fitted kernel, from a kept factor
 *   S3  HT @ alpha                       treegp/gp_interp.py:177,183
 *   S3b posterior covariance             treegp/gp_interp.py:184-192
 *   S3c posterior variance               treegp/gp_interp.py:184-192, as the reference's tests use it: np.diag(y_cov)
 *   S3d realisations y = L z             np.random.multivariate_normal(0, K) at tests/treegp_test_helper.py:64-66, 95-97
 *   S3e diag(K^-1) of a kept factor      not in the reference: leave-one-out residuals and variances (R&W 5.4.2)
 *   S3g gradient of HT @ alpha           not in the reference: d/dX2 of treegp/gp_interp.py:177,183 (kernels.py:114-126, 249-276, 355-381)
 *   S3l local kriging                    not in the reference: treegp/gp_interp.py:177-192 on each query's k nearest stars, no n x n factor
 *   S3v local conditionals               not in the reference: S3l at the training rows themselves (leave-one-out, Vecchia's log L)
 *   S3f many small S3b / S3c at once    treegp/gp_interp.py:184-192 for the problems of S2e, README.rst:28
 *   S4  treecorr KKCorrelation.process   treegp/two_pcf.py:297-305, 330-334, 342-362
 *   S5  KNeighborsRegressor.predict      treegp/gp_interp.py:236-238
 *   S6  binned_statistic_2d              treegp/meanify.py:76-107
 *   S7  vcorr pair accumulation          treegp/utils.py:36-72
 * followed by a device-resident tier (bench, tests) and the multi-GPU tier driven by treegp_amd/dist.py.
 *
 * Conventions
 *   - plain C types only; every array is C-contiguous float64 (or int64 where named so).
 *   - pointers are HOST pointers unless the parameter name starts with d_ (device pointer).
 *     The library never keeps a host pointer after the call returns.
 *   - coordinates are always passed as (n, 2) row-major; 1-D problems pass a zero second
 *     column (what treegp/two_pcf.py:250-251 does for the pair counter).
 *   - return 0 = ok; > 0 = LAPACK-style "leading minor of order i is not positive definite"
 *     (the Python shim raises numpy.linalg.LinAlgError, as scipy.linalg.cholesky does at
 *     gp_interp.py:181); < 0 = argument / HIP error, text in tgp_last_error().
 *   - a tgp_ctx owns one device, one stream and a grow-only workspace; it is not re-entrant.
 */
#ifndef TGP_H
#define TGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tgp_ctx tgp_ctx;
typedef struct tgp_factor tgp_factor;

/* kernel kinds (treegp/kernels.py + sklearn RBF); amp = sigma^2 of sklearn's
 * Product(ConstantKernel(sigma^2), k) folded in: value = amp * k(x, x').               */
enum {
    TGP_RBF = 0,      /* sklearn RBF(l): a = c = 1/l^2, b = 0 filled by the caller       */
    TGP_ARBF = 1,     /* AnisotropicRBF: exp(-0.5 q), q = a dx^2 + 2 b dx dy + c dy^2   */
    TGP_VK = 2,       /* VonKarman(l):  u = |d|/l                                       */
    TGP_AVK = 3       /* AnisotropicVonKarman: u = sqrt(q)                              */
};                    /* von Karman: u^(5/6) K_{5/6}(2 pi u) / lim0, 1 at u == 0        */

typedef struct {
    int32_t kind;
    int32_t _pad;
    double amp;       /* sigma^2                                                       */
    double a, b, c;   /* invLam[0,0], invLam[0,1], invLam[1,1]                          */
    double ell;       /* VonKarman length_scale                                         */
} tgp_kernel;

/* ---- context ------------------------------------------------------------------------ */
/* One context = one GPU: ndev must be 1.  SURVEY 8(b)'s "one process drives the node's GPUs" (ndev > 1) is served one level up:
 * treegp_amd/dist_pool.py starts one worker process per GPU, each with a context of its own and an RCCL group among them, behind
 * GPInterpolation(backend="dist") in an ordinary single-process script; the tgp_dd_* entry points below are the
 * per-rank building blocks those workers (and torchrun ranks) call.                                                          */
int tgp_init(const int *devices, int ndev, tgp_ctx **out);
void tgp_destroy(tgp_ctx *ctx);
const char *tgp_last_error(tgp_ctx *ctx);
const char *tgp_version(void);
int tgp_device_count(void);

/* phase timings (ms, hipEvent on the ctx stream) of the last call that recorded them:
 * [0] K build  [1] Cholesky total  [2] triangular solves  [3] predict  [4] pair binning
 * [5] trailing-update (syrk) kernel time summed  [6] number of trailing-update launches
 * [7] trailing-update flops (sum over launches)  [8] K-build bytes written
 * [9] result transfer of tgp_gp_predict_cov / tgp_gp_predict_var ([3] is then its device compute time)
 * [10] triangular sweeps over L inside [2]: 2 = forward + backward, 1 = backward only (the forward substitution
 *      rode along with the factorisation, inside [1]), 0 = none (likelihood only, right-hand side as a matrix row)
 * [11] device time of the product L Z of tgp_factor_lmul (transfers excluded)                                     */
#define TGP_NTIMINGS 12
int tgp_last_timings(tgp_ctx *ctx, double *ms, int n);
/* when on (default off) the Cholesky brackets every trailing-update launch with events */
int tgp_set_profiling(tgp_ctx *ctx, int on);
/* 0: the factorisation of this context stays on its one stream (no look-ahead on the side stream).  For contexts
 * that run side by side -- e.g. the independent likelihood evaluations of one finite-difference gradient
 * (treegp/log_likelihood.py:57 lets SciPy take them one after the other): hardware queues are few.          */
int tgp_set_lookahead(tgp_ctx *ctx, int on);

/* ---- S1: kernel matrix (host buffers) --------------------------------------------------
 * out (n, m) row-major = amp * k(X_i, Y_j).  Y == NULL: self kernel, out is (n, n) and the
 * diagonal is exactly amp (kernels.py:121,261,367).                                      */
int tgp_kernel_matrix(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n,
                      const double *Y, int64_t m, double *out);

/* ---- S2: alpha = (K + diag(yerr^2))^-1 y, logdet = sum 2 log diag(chol) ------------------
 * K never leaves the device.  keep != NULL receives a handle on the device-resident factor
 * (free with tgp_factor_free).  alpha may be NULL (log-likelihood only needs y.alpha, which
 * is returned in *ydota when ydota != NULL; it is then computed as |L^-1 y|^2, with y carried
 * through the factorisation as an extra row of the matrix, or from the forward sweep alone).  */
int tgp_gp_solve(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n,
                 const double *y, const double *yerr, double *alpha, double *logdet,
                 double *ydota, tgp_factor **keep);
void tgp_factor_free(tgp_ctx *ctx, tgp_factor *f);
/* gives the handle up but leaves its device memory with the context as the factor cache of the next solve of the same size
 * (no hipFree + hipMalloc of the packed matrix between two fits of one size); freed by tgp_destroy or a solve of another size */
void tgp_factor_release(tgp_ctx *ctx, tgp_factor *f);
/* the context gives back the device memory it holds between calls (factor cache, inverse slabs, scratch); they are allocated
 * again on demand.  For a process that is about to allocate elsewhere on the same GPU.                                     */
int tgp_release_caches(tgp_ctx *ctx);
/* a handle on a factor in the CALLER's device memory (d_A: tgp_panel_elems(Np) packed doubles, d_W: Np x 128, as
 * tgp_d_potrf leaves them) -- the multi-GPU driver's replicated factor; tgp_factor_free never frees d_A / d_W of it.
 * Serves the same reference lines as a kept factor: gp_interp.py:184-192 (covariance), README.rst:28 (several fields). */
int tgp_factor_borrow(tgp_ctx *ctx, double *d_A, double *d_W, int64_t n, tgp_factor **out);

/* ---- S2b: the same for a kernel matrix the CALLER evaluated ---------------------------------
 * For scikit-learn kernel trees tgp_kernel cannot describe (Sum, WhiteKernel, Matern, ...): the
 * reference evals any of them (treegp/kernels.py:17-59) and factorises what kernel(X1) returns
 * (treegp/gp_interp.py:180-182).  K: (n, n) row-major, its lower triangle is read; yerr^2 (may be
 * NULL) is added to the diagonal on the device.  Everything else as tgp_gp_solve.              */
int tgp_gp_solve_dense(tgp_ctx *ctx, const double *K, int64_t n, const double *y, const double *yerr,
                       double *alpha, double *logdet, double *ydota, tgp_factor **keep);

/* ---- S2c: more right-hand sides against a kept factor ("multi-field") -----------------------
 * One GP per field, all fields sharing the coordinates and the kernel (the Piff pattern the
 * reference names at README.rst:28; with the reference each field is its own GPInterpolation and
 * its own cholesky + cho_solve, gp_interp.py:180-182).  B and Xout: (nrhs, n) row-major;
 * Xout[v] = (K + diag(yerr^2))^-1 B[v].  The factor is read once per sweep for up to 4 fields.  */
int tgp_factor_solve(tgp_ctx *ctx, tgp_factor *f, const double *B, int nrhs, double *Xout);

/* ---- S2e: S2 for nb independent small problems in ONE launch sequence ------------------------------------------
 * The reference's regime is many small GPs: one per PSF parameter, exposure or chip (README.rst:28), each its own
 * cholesky + cho_solve (treegp/gp_interp.py:180-182), and 37-82 independent likelihood evaluations per maximum-likelihood
 * fit (treegp/log_likelihood.py:29-33, 43-62).  Problem b has its own kernel ks[b] (kinds may differ), order ns[b]
 * (1 <= ns[b] <= nmax <= 4096; above that one solve alone fills the chip: tgp_gp_solve), coordinates X (nb, nmax, 2),
 * values y (nb, nmax) and errors yerr (nb, nmax, or NULL); rows >= ns[b] are ignored.  Outputs: alpha (nb, nmax) or NULL,
 * entries >= ns[b] set to 0; logdet (nb); ydota (nb) = |L^-1 y|^2 or NULL; info (nb): 0, or > 0 = LAPACK-style order of
 * the failing minor of problem b, whose outputs are then meaningless -- the other problems' are unaffected, bit for bit.
 * A problem's bits depend neither on its companions, nor on its place in the batch, nor on the chunking: the batch runs
 * in chunks of as many problems as 90 % of the free device memory holds (TGP_BATCH_CHUNK problems per chunk overrides),
 * in the context's workspace (given back by tgp_release_caches).
 * Returns 0 when every problem was attempted; -1 for nb < 1, nmax > 4096, ns[b] out of range or an unknown kind; -2 for
 * HIP errors.  Timings [0] K build, [1] Cholesky, [2] sweeps and logdet, summed over the chunks; [10] sweeps (2, or 1
 * without alpha); every other slot 0.                                                                                  */
int tgp_gp_solve_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax, const double *X,
                       const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info);

/* ---- S2f: S2 and the likelihood gradient S2d for the nb problems of S2e, in the same call ------------------------------------
 * A maximum-likelihood fit (treegp/log_likelihood.py:43-62) evaluates the likelihood 37-82 times; with one GP per PSF
 * parameter, exposure or chip (README.rst:28) many such fits run side by side, and one call here is one evaluation of all of
 * them.  The batch of S2e is factorised and solved as tgp_gp_solve_batch does it and, in the same chunk, each problem's factor
 * and alpha give
 *   grad[b][0..3] = 1/2 sum_ij (alpha_i alpha_j - [K^-1]_ij) dK_ij/dp   for p = log amp, a, b, c
 * in the convention and element order of tgp_gp_loglik_grad.  ks, ns, nmax, X, y, yerr, logdet, ydota and info as
 * tgp_gp_solve_batch; logdet and ydota are bit for bit what it returns; a problem with info[b] > 0 has meaningless outputs and
 * the others are unaffected, bit for bit.  A problem's bits depend neither on its companions, nor on its place in the batch,
 * nor on the chunking (TGP_BATCH_CHUNK, as S2e; the chunk also holds L^-T and K^-1, Np x Np each, per problem).
 * Gaussian kernels only (TGP_RBF, TGP_ARBF): a von Karman kind anywhere in ks returns -1 with a message naming the entry.
 * Returns 0 when every problem was attempted; -1 for the argument errors of S2e; -2 for HIP errors.  Timings [0] K build,
 * [1] Cholesky, [2] sweeps and logdet, [3] inverse and reduction, summed over the chunks; every other slot 0.              */
int tgp_gp_solve_grad_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax,
                            const double *X, const double *y, const double *yerr,
                            double *logdet, double *ydota, double *grad, int32_t *info);

/* ---- S2g: S2 and diag(K^-1) for the nb problems of S2e, in the same call ------------------------------------------------------
 * Between fitting and interpolating, a pipeline with one GP per PSF parameter, exposure or chip (README.rst:28) validates each
 * fit and rejects outliers by leave-one-out (Rasmussen & Williams 5.4.2; not in the reference): that needs alpha and the
 * diagonal of the inverse alone, S3e for one kept factor at a time.  Here the batch of S2e is factorised and solved as
 * tgp_gp_solve_batch does it and, in the same chunk, each problem's factor gives
 *   invdiag[b][i] = [(K_b + diag(yerr_b^2))^-1]_ii = |L_b^-1 e_i|^2   for i < ns[b], exactly 0 for ns[b] <= i < nmax
 * from L_b^-T substituted on the device as in S2f, without its K^-1 (half of its flops behind the solve).  invdiag is
 * (nb, nmax) and must not be NULL.  ks, ns, nmax, X, y, yerr, alpha (may be NULL), logdet, ydota (may be NULL) and info as
 * tgp_gp_solve_batch, bit for bit; all four kernel kinds; a problem with info[b] > 0 has meaningless outputs and the others are
 * unaffected, bit for bit.  A problem's bits depend neither on its companions, nor on its place in the batch, nor on nmax, nor
 * on the chunking (TGP_BATCH_CHUNK, as S2e; the chunk also holds L^-T, Np x Np, and nmax doubles per problem).
 * Returns 0 when every problem was attempted; -1 for the argument errors of S2e or a NULL invdiag; -2 for HIP errors.
 * Timings [0] K build, [1] Cholesky, [2] sweeps and logdet, [3] substitution and norms, summed over the chunks; every other
 * slot 0.                                                                                                                      */
int tgp_gp_loo_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax,
                     const double *X, const double *y, const double *yerr,
                     double *alpha, double *invdiag, double *logdet, double *ydota, int32_t *info);

/* ---- S3: ys[j] = sum_i amp k(Xs_j, X_i) alpha_i, HT never materialised -------------------*/
int tgp_gp_predict(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n,
                   const double *alpha, const double *Xs, int64_t m, double *ys);

/* ---- S3g: gs[j] = sum_i alpha_i amp grad k(x - X_i) at x = Xs_j: the spatial derivative of S3 ---------------------------
 * Not in the reference, whose users difference predict() at shifted points.  The interpolated fields are PSF parameters and
 * astrometric displacements over a focal plane: divergence and curl of a displacement field (the map-level counterpart of the
 * E/B split of S7), local plate scale and shear, the slope of a PSF parameter across a chip.  gs is (m, 2) row-major.  With
 * (dx, dy) = Xs_j - X_i, q = a dx^2 + 2 b dx dy + c dy^2 and u = sqrt(q), a pair contributes
 *   Gaussian kinds    -alpha_i amp exp(-q / 2) (a dx + b dy, b dx + c dy)
 *   TGP_AVK           -alpha_i amp w(u) (a dx + b dy, b dx + c dy),  w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0
 *   TGP_VK            the same with a = c = 1 / ell^2, b = 0
 * and exactly 0 when u == 0: the von Karman profile has a cusp at the origin (1 - D u^(5/3)), the field has zero slope on a
 * star, and differencing predict() across one is wrong by more than rounding.  A 1-D problem (zero second column, b = c = 0,
 * or TGP_VK) gets a zero second column back.  Same decomposition as S3 (no (m, n) matrix, no atomics): the result is
 * bit-identical from run to run, and a query's two numbers depend on the training set and its own coordinates only -- not on
 * m, nor on its place among the queries.  Returns -1 for an unknown kind or n, m < 1, -2 for HIP errors; timings[3] is the
 * device time.                                                                                                             */
int tgp_gp_predict_grad(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n,
                        const double *alpha, const double *Xs, int64_t m, double *gs);

/* ---- S3l: local kriging -- every query conditioned on its kn nearest training points alone ----------------------------------------
 * Not in the reference, whose predict is one dense factorisation of the whole K + diag(yerr^2) (treegp/gp_interp.py:177-192) and
 * ends where that factor stops fitting on a GPU.  A prediction is determined, to all useful digits, by the stars within a few
 * correlation lengths: here the cost is linear in m, there is no n x n anything, and with the 2-point-correlation optimisers
 * (S4, any n, no factorisation) initialize -> solve -> predict_local is a complete pipeline for catalogues of 10^5 - 10^6 stars.
 * Definition.  k: one tgp_kernel of any of the four kinds; kn in 1 .. 128, clipped to n.
 *   metric       "nearest" = most correlated: Euclidean distance in u = R x, R^T R = invLam with R the upper-triangular 2 x 2
 *                Cholesky factor computed on the host (TGP_ARBF, TGP_AVK), R = I for TGP_RBF / TGP_VK; u0 = r00 x + (r01 y), u1 =
 *                r11 y, each product and sum rounded on its own; d2 = fl(fl(du0^2) + fl(du1^2)).
 *   S(j)         the kn training rows with the smallest d2 to query j, ties to the lower row index, nearest first.  The search
 *                is exact for every input (clustered, collinear, duplicated points, queries far outside the data).
 *   outputs      K_S = amp k(X_S, X_S) + diag(yerr_S^2) (diagonal exactly amp + yerr^2), k* = amp k(X_S, x*_j), both evaluated on the
 *                ORIGINAL coordinates by the evaluators of S1; L L^T = K_S, v = L^-1 k*, w = L^-1 y_S;
 *                ys[j] = v . w;  var[j] = amp - v . v, not clamped (the convention of S3c).
 *   failure      info[j] = 0, or the order of the first pivot that is not positive (NaN included); ys[j] and var[j] are then NaN
 *                and every other query is unaffected, bit for bit.
 *   independence a query's outputs depend on the training set, the kernel, kn and its own coordinates only: not on m, not on its
 *                place in Xs, not on the other queries, not on the chunking.
 * yerr may be NULL (no noise); var and nbr may be NULL.  nbr is (m, kn) row-major: S(j), original row indices; with kn > n the
 * entries from n on are -1.  info (m) must not be NULL.
 * On the device: a uniform grid over the bounding box of the whitened training points (mean occupancy of the order of kn / 4,
 * one cell along an axis of zero extent), rows sorted by cell with a counting sort on the host; one search launch (one query per
 * 64-lane workgroup: square rings of cells, the kn best in LDS, candidates merged by a bitonic sort, no bound on the number of
 * candidates) and one solve launch (one query per workgroup: K_S, k* and y_S in one LDS matrix of kn + 2 rows, factorised with
 * the right-hand sides carried along) per chunk of queries.  Chunks of 65 536 queries, TGP_LOCAL_CHUNK overrides; the bits do
 * not depend on the chunk.  Memory is O(n + chunk kn) in the context's workspace, checked against the free device memory
 * before anything runs (-2 with a message naming the bytes).
 * Returns 0 when every query was attempted; -1 with a message for a NULL pointer (ctx, k, X, y, Xs, ys, info), n < 1 or
 * n >= 2^31, m < 1, kn outside 1 .. 128, an unknown kind or an invLam without a Cholesky factor; -2 for HIP errors.
 * Timings: [0] grid build and upload (host wall clock), [2] neighbour search, [3] local solves, device time summed over the
 * chunks; every other slot 0.                                                                                                   */
int tgp_gp_predict_local(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n, const double *y, const double *yerr,
                         const double *Xs, int64_t m, int kn, double *ys, double *var, int32_t *nbr, int32_t *info);

/* ---- S3v: local conditionals -- every TRAINING row conditioned on its kn nearest eligible rows: local leave-one-out, Vecchia -------
 * Not in the reference.  The computation of S3l with the query x* = X[i] and a predicate on the candidate row in the search:
 * what judges or fits a kernel (likelihood, held-out score) without the dense factor, linear in n.
 * Definition.  k, X (2-D; 1-D as a zero second column), y, yerr, the metric, the whitening, d2 and the order of ties between
 * eligible rows (to the lower row index), lists nearest first: exactly S3l's.  kn in 1 .. 128.
 *   mode         TGP_LOCAL_LOO: the eligible rows of row i are all rows r != i -- by row index, not by coordinates: a duplicate
 *                of point i at another row is a legal neighbour, the first one.
 *                TGP_LOCAL_PRIOR: the rows with rank[r] < rank[i]; rank (n) must be a permutation of 0 .. n - 1, checked on the host
 *                in O(n) (-1 with a message naming the first offending entry).  sum_i log N(y_i | mu_i, var_i + yerr_i^2) is then
 *                Vecchia's approximation of log L, exact by the chain rule once kn reaches all predecessors.
 *   S(i)         the min(kn, number of eligible rows) nearest eligible rows; cnt[i] its length (0 for the first row of the
 *                ordering, or n = 1); the entries of nbr (n, kn) from cnt[i] on are -1.
 *   nbr_in       not NULL: the lists are taken from it, (n, kn) with -1 padding at the end only; no search runs, mode and rank are
 *                not consulted.  Checked on the host: every entry in [0, n) or a trailing -1, row i not in its own list (-1 with
 *                a message naming the row).  A row repeated within a list is not looked for: it surfaces as info[i] > 0.
 *   outputs      K_S, k* and the factorisation as in S3l with x* = X[i]: mu[i] = v . w, var[i] = amp - v . v (the LATENT variance,
 *                not clamped); with cnt[i] = 0, mu = 0 and var = amp.  info[i] as in S3l; mu and var are NaN on failure and every
 *                other row is unaffected, bit for bit.
 *   sums[3]      sums[0] = sum log s2_i, sums[1] = sum (y_i - mu_i)^2 / s2_i over the rows with info = 0, s2_i = var[i] + yerr_i^2
 *                (yerr^2 = 0 without yerr); sums[2] = the number of rows with info > 0.  The per-row terms are written to device
 *                arrays and reduced by launches of their own after the last chunk, in a fixed tree over the row index (blocks of
 *                1024: (e[t] + e[t+256]) + (e[t+512] + e[t+768]), a halving tree over t, then the same over the blocks): the bits
 *                do not depend on TGP_LOCAL_CHUNK.  No atomics.
 *   independence row i's outputs depend on the data, the kernel, kn, the mode or rank, and i only; not on the chunk.
 *   identities   LOO: row i is tgp_gp_predict_local on the training set without row i, queried at X[i]; PRIOR: on the rows of lower
 *                rank, kept in row order -- the same bits of mu and var, the same list after mapping the indices (the search is
 *                exact, the solve is the same operations in the same order).
 * mu, var, nbr, cnt and sums may each be NULL; info (n) must not be.  Memory is O(n + chunk kn), checked as in S3l (-2 with a
 * message naming the bytes); -1 / -2 as in S3l, also -1 for a mode that is neither.  On -1 no output is written.
 * Timings: [0] checks, grid build and upload (host wall clock), [2] neighbour search, [3] solves, terms and the reduction.      */
#define TGP_LOCAL_LOO 0
#define TGP_LOCAL_PRIOR 1
int tgp_gp_local_cond(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n, const double *y, const double *yerr,
                      int mode, const int32_t *rank, int kn, const int32_t *nbr_in,
                      double *mu, double *var, int32_t *nbr, int32_t *cnt, int32_t *info, double *sums);

/* ---- S3b: cov (m, m) = k(Xs,Xs) - HT K^-1 HT^T using a kept factor ------------------------*/
int tgp_gp_predict_cov(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X,
                       int64_t n, const double *Xs, int64_t m, double *cov);
/* the same with HT = kernel(X2, Y=X1) (m, n) and Kss = kernel(X2) (m, m) evaluated by the caller
 * (treegp/gp_interp.py:177,191 for kernel trees that go through tgp_gp_solve_dense)              */
int tgp_gp_predict_cov_dense(tgp_ctx *ctx, tgp_factor *f, const double *HT, const double *Kss,
                             int64_t m, double *cov);

/* ---- S3c: posterior variance, the diagonal of S3b without the (m, m) matrix -------------------
 * Every caller of predict(X, return_cov=True) in the reference keeps only np.diag(y_cov) (its tests, e.g.
 * tests/test_gp_interp.py:51-52).  var (m) = diag(k(Xs,Xs) - HT K^-1 HT^T) from a kept factor; any m (processed in
 * chunks of query rows: TGP_VAR_CHUNK rows, rounded up to 256, overrides the default; the result does not depend on
 * the chunk).  Not clamped at zero.  Timings as tgp_gp_predict_cov: [3] device compute, [9] result transfer.      */
int tgp_gp_predict_var(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                       const double *Xs, int64_t m, double *var);
/* the same with HT = kernel(X2, Y=X1) (m, n) and kss = kernel.diag(X2) (m) evaluated by the caller */
int tgp_gp_predict_var_dense(tgp_ctx *ctx, tgp_factor *f, const double *HT, const double *kss,
                             int64_t m, double *var);

/* ---- S3f: S3b / S3c for the nb problems of S2e, from their factors, in the same call ------------------------------------
 * Every reference test and the documented usage call predict(X, return_cov=True) (treegp/gp_interp.py:184-192); with one GP
 * per PSF parameter, exposure or chip (README.rst:28) that is one factorisation and one substitution per object.  Here the
 * batch of S2e is factorised as tgp_gp_solve_batch does it and, in the same chunk, each problem's factor gives the posterior at
 * its ms[b] query points Xs (nb, mmax, 2) (rows >= ms[b] are not read): what = 1, unc (nb, mmax) = the variance as S3c;
 * what = 2, unc (nb, mmax, mmax) = the covariance as S3b.  Every entry outside ms[b] (variance) or ms[b] x ms[b] (covariance)
 * is exactly 0.  ks, ns, nmax, X, y, yerr, alpha, logdet, ydota and info as tgp_gp_solve_batch, bit for bit; a problem with
 * info[b] > 0 has meaningless outputs and the others are unaffected, bit for bit.  A problem's bits depend neither on its
 * companions, nor on its place in the batch, nor on the chunking (TGP_BATCH_CHUNK, as S2e; the chunk also holds Bt (Mp x Np,
 * Mp = mmax rounded up to 256) and, for the covariance, an Mp x Mp matrix per problem).  Not clamped at zero.
 * Limits: 1 <= ms[b] <= mmax; mmax <= 4096 for the covariance, <= 65 280 for the variance; nmax, ns and kinds as S2e.
 * Returns 0 when every problem was attempted; -1 with a message naming the entry for out-of-range arguments or an unknown
 * `what`; -2 for HIP errors.  Timings [0] K build, [1] Cholesky, [2] sweeps and logdet, [3] posterior device compute,
 * [9] result transfer, summed over the chunks; every other slot 0.                                                          */
int tgp_gp_posterior_batch(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax,
                           const double *X, const double *y, const double *yerr,
                           const int64_t *ms, int64_t mmax, const double *Xs, int what,
                           double *alpha, double *unc, double *logdet, double *ydota, int32_t *info);

/* ---- S3d: realisations -- Yout[v] = L Z[v], L the lower Cholesky factor of K + diag(yerr^2) kept by tgp_gp_solve /
 * tgp_gp_solve_dense (stands in for np.random.multivariate_normal(0, K) at tests/treegp_test_helper.py:64-66,95-97 of
 * the reference).  Z, Yout: (nrhs, n) row-major host.  L is read once per group of 8 right-hand sides; no atomics: the
 * result is bit-identical from run to run, and row v of Yout does not depend on the other rows of Z.
 * Device time in timings[11].                                                                                          */
int tgp_factor_lmul(tgp_ctx *ctx, tgp_factor *f, const double *Z, int nrhs, double *Yout);

/* ---- S3e: diag(K^-1) -- the leave-one-out quantities of a GP (Rasmussen & Williams 5.4.2, eqs. 5.10-5.12) need
 * alpha = K^-1 r and this diagonal alone.  d (n) = diag((K + diag(yerr^2))^-1) from a factor kept by tgp_gp_solve /
 * tgp_gp_solve_dense / tgp_factor_borrow: d_i = |L^-1 e_i|^2, identity rows substituted on the device in chunks of
 * TGP_INVDIAG_CHUNK rows (rounded up to the substitution's step, 1024 or 256), each from its own first column on
 * (~n^3 / 3 flops in all, no n x n buffer).  The result does not depend on the chunk.
 * Timings: [3] device compute, [9] transfer, each summed over the chunks.                                              */
int tgp_factor_inv_diag(tgp_ctx *ctx, tgp_factor *f, double *d);

/* ---- S3h: diagonal blocks of K^-1 -- what leaving a GROUP of points out of a GP needs (R&W 5.4.2 with blocks for points:
 * with P = (K + diag(yerr^2))^-1 and alpha = P r, the points G predicted from all the others have mean r_G - P_GG^-1 alpha_G,
 * covariance P_GG^-1 and log p(y_G | y_-G) = -g/2 log 2 pi + 1/2 log det P_GG - 1/2 alpha_G^T P_GG^-1 alpha_G).
 * Group g is rows [starts[g], starts[g+1]) of the problem of a factor kept by tgp_gp_solve / tgp_gp_solve_dense /
 * tgp_factor_borrow: starts holds ngroups + 1 strictly increasing values, starts[0] == 0, starts[ngroups] == n, every group at
 * most TGP_INVBLOCK_GMAX rows.  blocks receives the groups' blocks one after the other, block g a row-major g x g array at
 * offset sum_{h<g} g_h^2; both triangles are written and are equal bit for bit.  [P]_ij = Bt_i . Bt_j over the rows of
 * Bt = L^-T that S3e makes (same chunks of identity rows, TGP_INVDIAG_CHUNK raised to the largest group plus one step; a group
 * never straddles two chunks), summed on the fp64 matrix cores from the panel that holds the group's first row: ~n^3 / 3
 * flops of substitution plus sum g^2 (n - starts[g]), no n x n buffer, no atomics.  A block's bits depend neither on the
 * chunk nor on the other groups.  Returns -1 with a message naming the entry for a NULL pointer, ngroups < 1, starts that do
 * not increase or do not span [0, n], or a group above the limit (nothing has run on the device then); -2 for HIP errors.
 * Timings: [3] device compute, [9] transfer, each summed over the chunks.                                              */
#define TGP_INVBLOCK_GMAX 4096
int tgp_factor_inv_blocks(tgp_ctx *ctx, tgp_factor *f, const int64_t *starts, int64_t ngroups, double *blocks);

/* ---- S2d: gradient of the log marginal likelihood from a kept factor and its alpha ---------
 * (the reference's optimiser passes no jac, treegp/log_likelihood.py:57 -- this is what a caller who wants one
 * gets, in the kernel-derivative convention of treegp/kernels.py:128-150.)
 *   grad[0..3] = 1/2 sum_ij (alpha_i alpha_j - [K^-1]_ij) dK_ij/dp   for p = log amp, a, b, c   (b = invLam[0,1] = invLam[1,0])
 * Gaussian kernels only (TGP_RBF, TGP_ARBF): -1 with a message for the von Karman kinds.  K^-1 is formed on the device
 * (2/3 n^3 flops, two n x n buffers) and never leaves it.                                                             */
int tgp_gp_loglik_grad(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                       const double *alpha, double *grad);
/* K build + factorisation + solve + the gradient above in one call, for X (n, 2), y, yerr (may be NULL) that live on the
 * device (tgp_dev_alloc / tgp_h2d): what one evaluation of a gradient-driven fit needs; the factor is not kept.        */
int tgp_d_gp_solve_grad(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_y,
                        const double *d_yerr, double *logdet, double *ydota, double *grad);

/* ---- S2h: S2d and S2f for all four kernel kinds: the exact likelihood gradient of the von Karman kernels ------------------
 * Not in the reference: kernels.py:278-288 (VonKarman returns K times the distances, the derivative of nothing), 383-384
 * (AnisotropicVonKarman raises "Gradient can not be evaluated"), so its fits of the atmospheric kernels difference the
 * likelihood, ntheta + 1 factorisations per iteration.  With (dx, dy) = X_i - X_j, q = a dx^2 + 2 b dx dy + c dy^2, u = sqrt(q)
 * (TGP_VK: a = c = 1 / ell^2, b = 0, u = |d| / ell as the value evaluates it), K_ij = amp f(u), f the profile of
 * bessel_k56.h, w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0 (bessel_k16.h, as S3g) and
 * m_ij = alpha_i alpha_j - [K^-1]_ij:
 *   grad[0] =  1/2 sum_ij m_ij amp f(u_ij)            (diagonal: amp)
 *   grad[1] = -1/4 sum_ij m_ij amp w(u_ij) dx^2
 *   grad[2] = -1/2 sum_ij m_ij amp w(u_ij) dx dy
 *   grad[3] = -1/4 sum_ij m_ij amp w(u_ij) dy^2
 * for p = log amp, a, b, c in the convention and element order of S2d: its sums with exp(-q / 2) replaced by f in slot 0 and by
 * w in slots 1 .. 3.  A pair of distinct points at u == 0 adds f = 1 to slot 0 and exactly 0 to the others (w(0) is infinite
 * and never evaluated); beyond the value's cutoff (2 pi u > 697.87) f and w are exactly 0.  For TGP_VK the caller maps the
 * four numbers to theta = log ell with the row [0, -2 / ell^2, 0, -2 / ell^2] (kernels.spec_jacobian).
 * Arguments, limits, return codes, timings and chunking are those of the namesakes (S2d, S2f); an unknown kind returns -1 with
 * a message naming the entry.  For TGP_RBF / TGP_ARBF the results are bit for bit the namesakes': the same kernels, the same
 * launches.  In the batch the kinds may be mixed; a problem's bits depend neither on its companions (of whatever kind), nor on
 * its place, nor on the chunking; logdet / ydota are tgp_gp_solve_batch's; a problem with info[b] > 0 leaves the others
 * untouched.  The pair sum is O(n^2) beside the O(n^3) inverse: one exact evaluation costs the same ~3 factorisations'
 * worth of flops for every kind.                                                                                            */
int tgp_gp_loglik_grad_any(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                           const double *alpha, double *grad);
int tgp_d_gp_solve_grad_any(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_y,
                            const double *d_yerr, double *logdet, double *ydota, double *grad);
int tgp_gp_solve_grad_batch_any(tgp_ctx *ctx, int nb, const tgp_kernel *ks, const int64_t *ns, int64_t nmax,
                                const double *X, const double *y, const double *yerr,
                                double *logdet, double *ydota, double *grad, int32_t *info);

/* ---- S1s / S2s: sums of 2 .. TGP_SUM_MAX parametrised kernels, evaluated on the device ------------------------------------------
 * The reference knows sums only through treegp/kernels.py:17-59: eval_kernel evals ANY scikit-learn tree, e.g.
 * "0.3**2 * AnisotropicVonKarman(...) + 0.5**2 * AnisotropicRBF(...)", and gp_interp.py:177-192 works with the n x n (and M x n)
 * matrices that kernel(X1[, X2]) returns on the host.  Here the n x n matrix never visits the host: the kernels that STORE kernel
 * values (packed K build, cross panels of the posterior, dense kernel matrix) evaluate every term in registers and store the sum
 * once; everything that only consumes kernel values is linear in the kernel and runs the single-kernel launches once per term.
 * Rounding: an off-diagonal element is ((v_0 + v_1) + v_2) + v_3, plain fp64 adds in term order, v_t carrying exactly the bits the
 * single-kernel entry writes for term t (the amplitude multiply is rounded before the add); the diagonal of a self matrix is
 * ((amp_0 + amp_1) + ...) exactly, plus yerr_i^2 in the K build.  With nterms == 1 every entry IS its namesake: the same bits.
 * Each entry mirrors its namesake's arguments, limits, return codes and timings with a tgp_kernel_sum in place of the tgp_kernel;
 * nterms < 1, nterms > TGP_SUM_MAX or an unknown kind in any term returns -1 with a message naming the entry, before anything
 * runs on the device.  A factor kept by tgp_gp_solve_sum is an ordinary tgp_factor: tgp_factor_solve, _lmul, _inv_diag and
 * _inv_blocks serve it unchanged.
 * tgp_gp_predict_sum / tgp_gp_predict_grad_sum: the per-term results of S3 / S3g against the same alpha, added on the device in term
 * order (bit for bit the host sum of the namesakes' outputs).  tgp_gp_loglik_grad_sum: grad is (nterms, 4) row-major, row t =
 * d log L / d (log amp_t, a_t, b_t, c_t) in the convention of S2h; K^-1 is formed once and the pair pass of S2h runs once per
 * term (row t is bit for bit tgp_gp_loglik_grad_any of term t with the same factor and alpha).                                */
#define TGP_SUM_MAX 4
typedef struct {
    int32_t nterms;
    int32_t _pad;
    tgp_kernel term[TGP_SUM_MAX];
} tgp_kernel_sum;
int tgp_kernel_matrix_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *X, int64_t n, const double *Y, int64_t m,
                          double *out);
int tgp_d_kbuild_lower_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *d_X, int64_t n, const double *d_yerr,
                           double *d_A);
int tgp_gp_solve_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *X, int64_t n, const double *y, const double *yerr,
                     double *alpha, double *logdet, double *ydota, tgp_factor **keep);
int tgp_gp_predict_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *X, int64_t n, const double *alpha,
                       const double *Xs, int64_t m, double *ys);
int tgp_gp_predict_grad_sum(tgp_ctx *ctx, const tgp_kernel_sum *k, const double *X, int64_t n, const double *alpha,
                            const double *Xs, int64_t m, double *gs);
int tgp_gp_predict_cov_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                           const double *Xs, int64_t m, double *cov);
int tgp_gp_predict_var_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                           const double *Xs, int64_t m, double *var);
int tgp_gp_loglik_grad_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                           const double *alpha, double *grad /* nterms x 4 */);

/* ---- S2j: Fisher information of the hyper-parameters from a kept factor -------------------------------------------------------
 * Not in the reference, whose fits return a point estimate.  For the Gaussian likelihood
 *   F_ij = 1/2 tr(C dK/dp_i C dK/dp_j),   C = (K + diag(yerr^2))^-1,
 * and F^-1 is the covariance of the maximum-likelihood estimate; F does not depend on y.  The parameters are the device's own,
 * as in S2d / S2h: p_t = (log amp_t, a_t, b_t, c_t) for term t (TGP_VK: a = c = 1 / ell^2, b = 0), P = 4 nterms of them in term
 * order; the chain rule to theta stays on the host (kernels.fisher_theta: J F J^T with the Jacobians of the gradient).  With
 * g = amp exp(-q / 2) for the Gaussian kinds and g = amp w(u) for the von Karman kinds (q, u, f, w as in S2h) the derivative
 * matrices of a term are
 *   D_0 = amp f(u)  (the kernel values without noise, diagonal exactly amp),  D_1 = -1/2 g dx^2,  D_2 = -g dx dy,  D_3 = -1/2 g dy^2,
 * D_1 .. D_3 exactly zero on the diagonal, at an off-diagonal pair with u == 0 (where f = 1) and beyond the von Karman cutoff:
 * the pair arithmetic of S2h, value for value.  With L the kept factor, S_r = L^-1 D_r L^-T and F[r][s] = 1/2 <S_r, S_s>.
 * On the device: the D_r of a term in one launch (f and w once per pair), then per matrix the block substitution of S3b
 * (Y = D L^-T, both its 128-block and its big-step form, unchanged), a transpose in the panel layout (D is symmetric, so
 * Y^T = L^-1 D) and the substitution again; the sums over i, j < n as per-workgroup partial sums added by one workgroup in a
 * fixed order, no atomics.  About 8 nterms n^3 flops, 24 nterms factorisations' worth.
 * f: a factor kept by tgp_gp_solve / tgp_gp_solve_sum for the same X, kernel and yerr; it is only read (its inverse slabs are
 * built on first use, as for S3b).  fisher: P x P doubles, row-major.
 * Memory: P + 1 arrays of padded_n(n)^2 doubles plus the substitution's staging, in the context's scratch arenas.  If that
 * exceeds the free device memory the call returns -2 with a message naming the entry and the bytes needed, before anything
 * runs; there is no chunked form.  n != f->n, a NULL pointer, an unknown kind or nterms outside 1 .. TGP_SUM_MAX returns -1 with
 * a message naming the entry and the field, before any device work.  Timings: [3] device compute.
 * Promises: the same call gives the same bits, whatever the context did before; F[r][s] and F[s][r] carry the same bits; with
 * nterms == 1 tgp_gp_fisher_sum IS tgp_gp_fisher, the same launches and the same bits; the factor serves every other entry
 * afterwards exactly as before (tgp_gp_predict_var on it gives the same bits before and after).                             */
int tgp_gp_fisher(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel *k, const double *X, int64_t n,
                  double *fisher /* 4 x 4 */);
int tgp_gp_fisher_sum(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel_sum *k, const double *X, int64_t n,
                      double *fisher /* (4 nterms) x (4 nterms), row-major */);

/* ---- S2i: the batched routes (S2e, S2f / S2h, S2g, S3f) for sums of kernels ---------------------------------------------------
 * The reference's regime is many small GPs, and its most physical kernel is a sum (an atmospheric term plus a long-range optical
 * one): one tgp_kernel_sum per problem, ks [nb], 1 .. TGP_SUM_MAX terms each, term counts and kinds differing freely between the
 * problems of a batch.  Nothing below the K values knows what kernel built K, so factorisation, sweeps, substitution and
 * products are the launches of the namesakes; three device parts are the sums' own:
 *   K build      one 128 x 128 tile per workgroup as in S2e, every term evaluated in registers, the tile stored once;
 *   posterior    the cross panels H_b (and Kss_b) the same way; the prior variance is tgp_ksum_amp(k_b);
 *   gradient     K_b^-1 is formed once per problem; the pair pass of S2h runs once per term, over the problems whose term t has
 *                the launch's evaluator, into partial sums of their own; the fixed-order reduction runs per (problem, term).
 * Rounding, as in S1s / S2s: a strict-lower element of K_b (an element of H_b, an off-diagonal one of Kss_b) is
 * ((v_0 + v_1) + v_2) + v_3, plain fp64 adds in term order, v_t bit for bit what the one-term batched build writes for term t
 * (the amplitude multiply is rounded before the add); the diagonal of K_b is tgp_ksum_amp(k_b) + yerr_i^2, that of Kss_b exactly
 * tgp_ksum_amp(k_b); padding rows and columns are the single-kernel build's.
 * Launch lists: the problems of a chunk are grouped by what their own kernel needs -- one term: the evaluator's launch of the
 * namesake; two or more Gaussian terms: an instantiation that carries no Bessel evaluator; a sum with a von Karman term: one that
 * does.  A problem's list is decided by its kernel alone.
 * Each entry has its namesake's arguments, limits, return codes, timings and chunking with const tgp_kernel_sum *ks in place of
 * const tgp_kernel *ks.  tgp_gp_solve_grad_batch_sum is tgp_gp_solve_grad_batch_any with grad (nb, TGP_SUM_MAX, 4): row t of
 * problem b is d log L / d (log amp_t, a_t, b_t, c_t) in the convention of S2h, rows t >= nterms_b are exactly 0.
 * tgp_kbuild_batch_sum is the building block: it stages the batch, runs the batched K build at the batch's common Np and returns
 * every problem's lower triangle with its diagonal, row-major in its nmax x nmax slot of K (nb, nmax, nmax); everything above
 * the diagonal or beyond ns[b] is exactly 0.  No factorisation runs.  It is to the batch what tgp_d_kbuild_lower +
 * tgp_d_unpack_lower are to the single solve; yerr may be NULL; timings [0] K build, every other slot 0.
 * Argument errors: nterms outside 1 .. TGP_SUM_MAX or an unknown kind in any term of any problem returns -1 with a message
 * naming the entry, the problem and the term, before anything runs on the device; the others are those of S2e.
 * Promises: with nterms == 1 everywhere every entry IS its namesake, the same launches and the same bits.  A problem's bits
 * depend neither on its companions, whatever their term counts and kinds, nor on its place, nor on the chunking
 * (TGP_BATCH_CHUNK), nor on nmax wherever the namesake promises that.  A problem with info[b] > 0 leaves the others untouched,
 * bit for bit.                                                                                                              */
int tgp_gp_solve_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax, const double *X,
                           const double *y, const double *yerr, double *alpha, double *logdet, double *ydota, int32_t *info);
int tgp_gp_posterior_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax,
                               const double *X, const double *y, const double *yerr,
                               const int64_t *ms, int64_t mmax, const double *Xs, int what,
                               double *alpha, double *unc, double *logdet, double *ydota, int32_t *info);
int tgp_gp_loo_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax,
                         const double *X, const double *y, const double *yerr,
                         double *alpha, double *invdiag, double *logdet, double *ydota, int32_t *info);
int tgp_gp_solve_grad_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax,
                                const double *X, const double *y, const double *yerr,
                                double *logdet, double *ydota, double *grad /* (nb, TGP_SUM_MAX, 4) */, int32_t *info);
int tgp_kbuild_batch_sum(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax,
                         const double *X, const double *yerr, double *K);

/* ---- S1, S2, S3 in three dimensions --------------------------------------------------------------------------------------------
 * The reference's kernels take coordinates of any dimension (treegp/kernels.py:114-126, 355-381 hand pdist / cdist whatever invLam
 * they are given; VonKarman and scikit-learn's RBF use Euclidean distances): position plus time, position plus colour.  These
 * entries are their namesakes with X and Xs in (n, 3) / (m, 3) row-major and the kernel as a tgp_kernel3:
 *   m       the upper triangle of the symmetric invLam, row-wise: xx, xy, xz, yy, yz, zz.  d^T invLam d is evaluated as
 *           xx dx dx + 2xy dx dy + 2xz dx dz + yy dy dy + 2yz dy dz + zz dz dz from the differences d.  TGP_RBF: xx, yy, zz =
 *           1 / l^2 per axis, the rest 0.  TGP_VK ignores m: u = |d| / ell.
 * Only the launches that EVALUATE a kernel are the 3-D entries' own (nd3.hip): the packed K build (the layout, padding and exact
 * diagonal amp + yerr_i^2 of S2), the dense kernel matrix (self: diagonal exactly amp), the fused mean and its gradient (the
 * decomposition of S3 / S3g: 256 training points per LDS tile, partial sums per split, fixed-order reduce, no atomics; the
 * Gaussian kinds through coordinates transformed once per call by the Cholesky factor of invLam, the direct quadratic form when
 * invLam has none) and the cross panels of the posterior.  Factorisation, sweeps, substitution and products are the namesakes'
 * launches: a factor kept by tgp_gp_solve3 is an ordinary tgp_factor, and tgp_factor_solve, _lmul, _inv_diag and _inv_blocks serve
 * it unchanged.  The amplitude is multiplied after the transcendental; coincident points give exactly amp; a von Karman pair
 * beyond 2 pi u > 697.87 is exactly 0; a pair at u == 0 contributes exactly 0 to the gradient; a NaN coordinate or parameter stays
 * NaN.  tgp_gp_predict_grad3: gs is (m, 3).  tgp_gp_predict_var3 is the diagonal of tgp_gp_predict_cov3 (same panels, same
 * substitution).  Arguments, limits, return codes and timings are the namesakes'; ndim != 3 or an unknown kind returns -1 with
 * a message naming the entry and the field, before anything runs on the device.
 * tgp_d_kbuild_lower3 is the building block, as tgp_d_kbuild_lower: d_X (n, 3) and d_A on the device; with tgp_d_unpack_lower it
 * makes the stored values testable pair by pair.                                                                              */
typedef struct {
    int32_t kind;     /* TGP_RBF, TGP_ARBF, TGP_VK, TGP_AVK, meanings unchanged */
    int32_t ndim;     /* 3 */
    double amp;
    double m[6];      /* invLam xx, xy, xz, yy, yz, zz (TGP_RBF: xx, yy, zz = 1 / l^2, the rest 0) */
    double ell;       /* TGP_VK: u = |d| / ell */
} tgp_kernel3;
int tgp_kernel_matrix3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *X, int64_t n, const double *Y, int64_t m, double *out);
int tgp_d_kbuild_lower3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *d_X, int64_t n, const double *d_yerr, double *d_A);
int tgp_gp_solve3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *X, int64_t n, const double *y, const double *yerr,
                  double *alpha, double *logdet, double *ydota, tgp_factor **keep);
int tgp_gp_predict3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *X, int64_t n, const double *alpha, const double *Xs,
                    int64_t m, double *ys);
int tgp_gp_predict_grad3(tgp_ctx *ctx, const tgp_kernel3 *k, const double *X, int64_t n, const double *alpha, const double *Xs,
                         int64_t m, double *gs /* (m, 3) */);
int tgp_gp_predict_cov3(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel3 *k, const double *X, int64_t n, const double *Xs,
                        int64_t m, double *cov);
int tgp_gp_predict_var3(tgp_ctx *ctx, tgp_factor *f, const tgp_kernel3 *k, const double *X, int64_t n, const double *Xs,
                        int64_t m, double *var);

/* ---- S4: binned scalar pair correlation, exact binning -----------------------------------
 * w == NULL: unit weights.  TwoD: nbins x nbins pixels over [-max_sep, max_sep]^2, outputs
 * of length nbins^2 (flat index iy*nbins+ix).  Log: nbins log-spaced bins in
 * [min_sep, max_sep).  xi = sum(w_i w_j k_i k_j)/sum(w_i w_j), 0 where the weight is 0.     */
int tgp_kk_twod(tgp_ctx *ctx, const double *x, const double *y, const double *k,
                const double *w, int64_t n, double min_sep, double max_sep, int nbins,
                double *xi, double *weight, double *npairs);
int tgp_kk_log(tgp_ctx *ctx, const double *x, const double *y, const double *k,
               const double *w, int64_t n, double min_sep, double max_sep, int nbins,
               double *xi, double *weight, double *meanr, double *meanlogr, double *npairs);
/* One shard of the same pair loop (multi-GPU, SURVEY 8e "pair histogram"): bin_type 0 = TwoD,
 * 1 = Log; the 256-point i-tiles are dealt round-robin to `nparts` callers and `part` bins
 * only its own.  acc_out holds the raw sums, 3 x nbins^2 (sum w w k k, sum w w, pairs) for
 * TwoD and 5 x nbins (sum wwkk, sum ww, sum ww r, sum ww ln r, pairs) for Log; adding the
 * shards (one all-reduce) and dividing by the weights gives tgp_kk_twod / tgp_kk_log.      */
int tgp_kk_partial(tgp_ctx *ctx, int bin_type, const double *x, const double *y, const double *k,
                   const double *w, int64_t n, double min_sep, double max_sep, int nbins,
                   int part, int nparts, double *acc_out);
/* bootstrap (two_pcf.py:269-281, 342-362): idx is (n_boot, n) int64; resample b uses points
 * idx[b,:], k = yv[idx] - mean(yv[idx]), w = 1/yerr[idx]^2 (unit weights if yerr == NULL or
 * sum(yerr[idx]) == 0).  xi_out is (n_boot, nbins^2).                                       */
int tgp_kk_twod_bootstrap(tgp_ctx *ctx, const double *x, const double *y, const double *yv,
                          const double *yerr, int64_t n, const int64_t *idx, int64_t n_boot,
                          double min_sep, double max_sep, int nbins, double *xi_out);

/* ---- vector 2-point correlation (E/B diagnostics): the pair accumulation of treegp/utils.py:5-74 ----
 * All pairs i < j; log|p_j - p_i| binned on `edges` (nbins + 1 increasing values = the uniform
 * edges np.histogram builds for (bins, range); last edge inclusive).  acc_out is (7, nbins):
 * pairs, sum log r, sum (dx_i dx_j + dy_i dy_j), Re and Im of sum v_i v_j (v = dx + i dy), Re and
 * Im of sum v_i v_j conj(d)^2/|d|^2.  xi_+ = acc[2]/acc[0], xi_- = acc[5]/acc[0], ...        */
int tgp_vcorr(tgp_ctx *ctx, const double *x, const double *y, const double *dx, const double *dy,
              int64_t n, const double *edges, int nbins, double *acc_out);

/* ---- mean function: uniform mean of the k nearest neighbours of each X in the table (X0, y0) -----
 * replaces KNeighborsRegressor(n_neighbors=k).fit(X0, y0).predict(X) at treegp/gp_interp.py:236-238.
 * k in 1..8 or 16.                                                                            */
int tgp_knn_mean(tgp_ctx *ctx, const double *X0, const double *y0, int64_t n0, const double *X, int64_t m,
                 int k, double *out);

/* ---- building the mean function ("meanify"): binned 2-D statistic of scattered values ------------
 * replaces scipy.stats.binned_statistic_2d(u, v, ., bins=[u_edges, v_edges], statistic=.) at
 * treegp/meanify.py:76-107, with scipy's bin numbering (np.digitize, last edge inclusive).
 * stat MEAN: sum/count; MEDIAN: scipy's median of the bin; WEIGHTED: w = 1/err^2,
 * average = sum(w p)/sum(w), wrms = sqrt((sum(w p p) - 2 avg sum(w p) + avg^2 sum(w))/sum(w)).
 * Outputs are (nu_edges-1, nv_edges-1) row-major (u index first, as scipy returns them; the
 * reference transposes afterwards); empty bins are NaN.  wrms (0 unless WEIGHTED) and count
 * (points per bin; sum of weights for WEIGHTED) may be NULL.                                  */
#define TGP_STAT_MEAN 0
#define TGP_STAT_MEDIAN 1
#define TGP_STAT_WEIGHTED 2
int tgp_binned_stat_2d(tgp_ctx *ctx, const double *u, const double *v, const double *val, const double *err,
                       int64_t n, const double *u_edges, int nu_edges, const double *v_edges, int nv_edges,
                       int stat, double *average, double *wrms, double *count);

/* ---- device-resident tier (bench / multi-GPU): same maths, d_ pointers, ctx stream --------*/
int tgp_dev_alloc(tgp_ctx *ctx, int64_t bytes, void **d_out);
int tgp_dev_free(tgp_ctx *ctx, void *d_ptr);
int tgp_h2d(tgp_ctx *ctx, void *d_dst, const void *src, int64_t bytes);
int tgp_d2h(tgp_ctx *ctx, void *dst, const void *d_src, int64_t bytes);
int tgp_sync(tgp_ctx *ctx);
void *tgp_stream(tgp_ctx *ctx);          /* the hipStream_t every kernel is launched on */
int tgp_mem_info(tgp_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);   /* device memory of the context's GPU */

/* d_X (n,2), d_y, d_yerr, d_alpha (n): resident inputs/outputs */
int tgp_d_gp_solve(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n,
                   const double *d_y, const double *d_yerr, double *d_alpha, double *logdet,
                   double *ydota, tgp_factor **keep);
int tgp_d_gp_predict(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n,
                     const double *d_alpha, const double *d_Xs, int64_t m, double *d_ys);
int tgp_d_gp_predict_grad(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n,
                          const double *d_alpha, const double *d_Xs, int64_t m, double *d_gs /* (m, 2) */);
/* d_K: dense (n, n) row-major on the device (lower triangle read) */
int tgp_d_gp_solve_dense(tgp_ctx *ctx, const double *d_K, int64_t n, const double *d_y,
                         const double *d_yerr, double *d_alpha, double *logdet, double *ydota,
                         tgp_factor **keep);

/* ---- factor storage: packed lower panels ("panel-major") -----------------------------------
 * Np = n rounded up to 256.  Panel p (p = 0 .. Np/256-1) holds rows 256p .. Np-1 of columns
 * 256p .. 256p+255, row-major with leading dimension 256; panels are stored back to back.
 * tgp_panel_elems(Np) doubles in total.  Element (i, j), i >= 256*(j/256):
 *   off = tgp_panel_off(j/256, Np) + (i - 256*(j/256))*256 + j%256                            */
int64_t tgp_panel_off(int64_t p, int64_t Np);
int64_t tgp_panel_elems(int64_t Np);
int64_t tgp_padded_n(int64_t n);

/* building blocks, exposed for parity tests, profiling and the multi-GPU driver */
int tgp_d_kbuild_lower(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n,
                       const double *d_yerr, double *d_A);
/* in-place Cholesky of the packed lower matrix; d_W receives (Np/128) inverted 128x128
 * diagonal blocks of L.  Returns 0 or the 1-based index of the first non-positive pivot. */
int tgp_d_potrf(tgp_ctx *ctx, double *d_A, int64_t Np, double *d_W);
/* d_b (Np) <- L^-T L^-1 d_b */
int tgp_d_potrs(tgp_ctx *ctx, const double *d_A, const double *d_W, int64_t Np, double *d_b);
/* d_B (nrhs, Np) row-major: every row <- L^-T L^-1 row */
int tgp_d_potrs_multi(tgp_ctx *ctx, const double *d_A, const double *d_W, int64_t Np, double *d_B, int nrhs);
/* unpack the lower triangle into a dense (n, n) row-major host matrix (upper part zero) */
int tgp_d_unpack_lower(tgp_ctx *ctx, const double *d_A, int64_t Np, int64_t n, double *out);
/* read-only view of a kept (or borrowed) factor: its packed panels, inverted blocks and Np; changes nothing */
int tgp_factor_device(tgp_ctx *ctx, const tgp_factor *f, const double **d_A, const double **d_W, int64_t *Np);
/* ---- multi-GPU tier (one process per GPU; driver: treegp_amd/dist.py) ------------------------
 * Row-block-cyclic over 256-row blocks with the deal reflected every G blocks: round q = b / G gives
 * rank g block q G + g when q is even and q G + (G-1-g) when q is odd, so that the lower triangle's
 * work (block row b carries b + 1 block columns) is even over the ranks.  A rank's local index of block
 * b is b / G; an all-gathered panel is [rank][cmax][256][256] with cmax = the most blocks any rank holds.
 * A rank's share of panel p (blocks b >= p) is stored like a single-GPU panel at element offset
 * tgp_dist_panel_off(p).  h_loff / d_loff are host / device copies of those offsets (Np/256+1
 * entries).  These calls only enqueue work on the context stream (tgp_set_stream points it at the
 * caller's stream so that RCCL collectives order with it); they replace, per panel, the same
 * reference lines as tgp_gp_solve (treegp/gp_interp.py:180-182).                              */
int tgp_set_stream(tgp_ctx *ctx, void *hip_stream);      /* launch on the caller's stream (NULL = default stream) */
int tgp_reset_stream(tgp_ctx *ctx);                      /* back to the context's own stream */
int tgp_set_side_stream(tgp_ctx *ctx, void *hip_stream); /* lend the look-ahead stream of the context's own schedules */
int64_t tgp_dist_panel_rows(int64_t p, int64_t Np, int G, int g);
int64_t tgp_dist_panel_off(int64_t p, int64_t Np, int G, int g);
int64_t tgp_dist_local_elems(int64_t Np, int G, int g);
int tgp_dd_kbuild(tgp_ctx *ctx, const tgp_kernel *k, const double *d_X, int64_t n, const double *d_yerr,
                  double *d_Aloc, const int64_t *d_loff, int G, int g);
/* owner of panel kpanel: factor the diagonal block, pack [L_kk(256x256) | W0 | W1] = 98304 doubles */
int tgp_dd_factor_diag(tgp_ctx *ctx, double *d_Aloc, const int64_t *h_loff, int64_t Np, int kpanel, int G, int g,
                       double *d_W, double *d_bcast);
/* every rank, after the broadcast of d_bcast: solve the local rows of panel kpanel (16-row slices while the rank holds at
 * most 24 row tiles, 128-row tiles above); a receiver's d_W gets the panel's inverted blocks from d_bcast by the same grid */
int tgp_dd_trsm(tgp_ctx *ctx, double *d_Aloc, const int64_t *h_loff, int64_t Np, int kpanel, int G, int g,
                double *d_W, const double *d_bcast);
/* every rank, after the all-gather of the panel ([rank][cmax][256][256]): update the local block rows,
 * trailing 128-tile columns [col_lo, col_hi) only (col_hi < 0: to the end) -- the first two columns are
 * the next panel, updated first so that its factorisation overlaps the rest (look-ahead)          */
int tgp_dd_update(tgp_ctx *ctx, double *d_Aloc, const int64_t *d_loff, int64_t Np, int kpanel, int G, int g,
                  const double *d_gathered, int cmax, int col_lo, int col_hi);
/* the same after the PAIR of panels (kpanel, kpanel+1) in one pass of depth 512: gathered0 / gathered1 are
 * the all-gathered panels kpanel (blocks > kpanel, cmax0 per rank) and kpanel+1 (blocks > kpanel+1, cmax1);
 * tile columns col_lo..col_hi count from block kpanel+2.                                              */
int tgp_dd_update2(tgp_ctx *ctx, double *d_Aloc, const int64_t *d_loff, int64_t Np, int kpanel, int G, int g,
                   const double *d_gathered0, int cmax0, const double *d_gathered1, int cmax1, int col_lo,
                   int col_hi);
/* general form: after the GROUP of nseg (1..4) consecutive panels kpanel .. kpanel+nseg-1 in one pass of depth
 * 256 nseg.  d_gathered[s] / cmax[s] (host arrays) describe the all-gathered panel kpanel+s (blocks > kpanel+s);
 * tile columns col_lo..col_hi count from block kpanel+nseg.  nseg = 1 and 2 are tgp_dd_update / tgp_dd_update2.   */
int tgp_dd_update_group(tgp_ctx *ctx, double *d_Aloc, const int64_t *d_loff, int64_t Np, int kpanel, int G, int g,
                        int nseg, const double *const *d_gathered, const int *cmax, int col_lo, int col_hi);
/* Panel chain with the panel exchange off it (dist.py, TGP_DIST_CHAIN_BCAST; the seam is the same treegp/gp_interp.py:180-182):
 * block b = kgroup + j of a group (1 <= j <= 3) against the j earlier panels of the group in one pass of depth 256 j, this rank's
 * rows of b's two tile columns.  Rows: the rank's own, where they are stored (h_loff: the host copy of d_loff).  Columns: block
 * b's rows of those panels, d_ext[s] (256 x 256 doubles, s = panel - kgroup), as appended by b's owner to the broadcast of its
 * diagonal block; NULL on the owner.  Reads no all-gathered panel.                                                         */
int tgp_dd_strip_left(tgp_ctx *ctx, double *d_Aloc, const int64_t *h_loff, const int64_t *d_loff, int64_t Np, int kgroup, int b,
                      int G, int g, const double *d_ext);
/* The bulk part of the update as a persistent grid that keeps `nres` (1..3) compute units per shader engine and XCD clear for
 * the panel chain (diagonal block, local solves, strips) that runs beside it on another stream; for the steps where this
 * rank's share of the bulk is shorter than the chain.  tgp_dd_queue_reset: once per factorisation, on the launching context;
 * tgp_dd_set_exclusive(chain ctx, 1): its diagonal blocks then take a compute unit of their own (44 us instead of ~170 us
 * beside bulk waves) -- only while such a launch keeps units clear.                                                        */
int tgp_dd_queue_reset(tgp_ctx *ctx);
int tgp_dd_set_exclusive(tgp_ctx *ctx, int on);
int tgp_dd_update_group_queued(tgp_ctx *ctx, double *d_Aloc, const int64_t *d_loff, int64_t Np, int kpanel, int G, int g,
                               int nseg, const double *const *d_gathered, const int *cmax, int col_lo, int col_hi, int nres);
/* the whole update after a group in ONE launch, the tile columns [0, head_cols) first; the launch publishes a flag when
 * they are done and tgp_dd_wait_head parks the stream of `waiter` (the panel chain's context) on it.  Only where
 * tgp_handoff_mode(ctx) == 1 (hand-offs by stream wait-value; 2 = events: split the update in two calls instead).   */
int tgp_dd_update_group_fused(tgp_ctx *ctx, double *d_Aloc, const int64_t *d_loff, int64_t Np, int kpanel, int G, int g, int nseg,
                              const double *const *d_gathered, const int *cmax, int head_cols, int nres);
int tgp_dd_wait_head(tgp_ctx *ctx, tgp_ctx *waiter);
/* replicated finish of the factorisation: after ONE all-gather of every rank's share of the trailing matrix from panel k0 on
 * (d_gathered: [G][stride] doubles, a rank's region exactly as it stores it), assemble the packed lower matrix of order
 * Np - 256 k0 at d_tail (the replicated factor's tail, or a buffer of tgp_panel_elems(Np - 256 k0)); the caller factors it
 * with tgp_d_potrf and tgp_dd_tail_scatter copies this rank's blocks of the result back into its share.               */
int tgp_dd_tail_assemble(tgp_ctx *ctx, const double *d_gathered, int64_t stride, int64_t Np, int k0, int G, double *d_tail);
int tgp_dd_tail_scatter(tgp_ctx *ctx, const double *d_tail, int64_t Np, int k0, int G, int g, double *d_Aloc, const int64_t *d_loff);
/* how this context's streams hand over to each other: 1 = flags + hipStreamWaitValue32, 2 = events (chosen by a first-use
 * trial per device, or TGP_SYNC_EVENTS=1 / 0) */
int tgp_handoff_mode(tgp_ctx *ctx);
/* Replicated factor for the solves: store panel kpanel into d_Afull, a full single-GPU packed matrix
 * (tgp_panel_elems(Np) doubles) kept on every rank -- its 256x256 diagonal block from the broadcast buffer
 * (d_bcast, may be NULL) and/or the rows below it from the all-gathered panel (d_gathered, may be NULL).
 * After the last panel, tgp_d_potrs(ctx, d_Afull, d_W, Np, rhs) solves on every rank without communication. */
int tgp_dd_keep_panel(tgp_ctx *ctx, double *d_Afull, int64_t Np, int kpanel, int G, const double *d_bcast,
                      const double *d_gathered, int cmax);
/* block-row-cyclic triangular solves (scipy cho_solve, gp_interp.py:182) */
int tgp_dd_fwd_diag(tgp_ctx *ctx, const double *d_Aloc, const int64_t *h_loff, int kb, const double *d_W, double *d_yk);
int tgp_dd_fwd_update(tgp_ctx *ctx, const double *d_Aloc, const int64_t *h_loff, int64_t Np, int kb, int G, int g,
                      const double *d_zk, double *d_yloc);
int tgp_dd_bwd_partial(tgp_ctx *ctx, const double *d_Aloc, const int64_t *h_loff, int64_t Np, int kb, int G, int g,
                       const double *d_aloc, double *d_s);
int tgp_dd_bwd_diag(tgp_ctx *ctx, const double *d_Aloc, const int64_t *h_loff, int kb, const double *d_W, double *d_ak,
                    const double *d_s /* subtracted from a_k first; may be NULL */);
int tgp_dd_logdet_local(tgp_ctx *ctx, const double *d_Aloc, const int64_t *d_loff, int64_t Np, int64_t n, int G, int g,
                        double *d_out);
int tgp_dd_info(tgp_ctx *ctx, int reset);                /* first non-PD pivot since the last reset */

/* measurement hook: `reps` launches of the depth-512 trailing update over a whole packed Np x Np
 * matrix (contents arbitrary), timed with HIP events on the context's stream */
int tgp_debug_syrk_loop(tgp_ctx *ctx, double *d_A, int64_t Np, int reps, double *ms_per_launch,
                        double *flops_per_launch);
/* test hook: tile enumeration of the trailing update over T x T 128-tiles; fills (ti, tj)
 * for every block id (-1 = empty slot) and returns the grid size, or -1 if cap is too small */
int tgp_debug_tilemap(int64_t T, int32_t *ti, int32_t *tj, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TGP_H */
