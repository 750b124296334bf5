"""The condition ladder's references, checked on the host: the inputs reach the condition numbers the GPU tests
(test_gpu_cond_ladder.py) claim to cover, LAPACK factors every rung, the long-double refinement converges, and LAPACK's own
solution is backward stable to n u.  LAPACK's figures per rung are printed (-s)."""
import numpy as np
import pytest

import _cond_ladder as CL

N = 2304


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("i", CL.RUNGS)
def test_rung_reaches_its_condition_number(i):
    X, y, e, K0, K = CL.rung(i, N)
    assert not K.flags.writeable and not K0.flags.writeable and not y.flags.writeable
    assert np.all(e == CL.NOISES[i]) and X.shape == (N, 2) and X.min() >= 0.0 and X.max() <= 1.0
    assert np.array_equal(np.diag(K), np.diag(K0) + e ** 2)                  # one rounding per diagonal entry, as the device
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal(K[off], K0[off])
    c = CL.cond2(K)
    print("rung %d noise %.0e cond_2 %.3e (recorded %.1e)" % (i, CL.NOISES[i], c, CL.COND_2304[i]))
    assert CL.COND_2304[i] / 2 <= c <= CL.COND_2304[i] * 2


@pytest.mark.parametrize("i", CL.RUNGS)
def test_lapack_factors_refinement_converges_and_lapack_is_backward_stable(i):
    ref = CL.reference(i, N)                                                  # cho_factor raises where LAPACK cannot factor
    CL.check_refinement(ref.corr, "rung %d" % i)
    lap = ref.lapack
    print("rung %d corrections %s | LAPACK eta %.2e pred %.2e resid %.2e y.alpha %.2e fwd %.2e" % (
        i, " ".join("%.1e" % c for c in ref.corr), lap["eta"], lap["pred"], lap["resid"], lap["ydota"], lap["fwd"]))
    assert lap["eta"] <= N * CL.U
    # the refined solution is a better solution than LAPACK's by the two digits the validity condition promises
    r_ref = np.abs(CL.matmul_ld(ref.K, ref.alpha) - ref.y).max()
    r_lap = np.abs(CL.matmul_ld(ref.K, ref.alpha_lapack) - ref.y).max()
    assert r_ref <= 1e-2 * r_lap


@pytest.mark.parametrize("i,with_block", [(0, False), (4, True)])
def test_posterior_references(i, with_block):
    """The references of the variance, diag(K^-1) and (top rung) the block are valid (refinement converges, checked inside) and
    LAPACK's figures for them are of the size cond u."""
    n = 1000 + 130 + 22                                                       # the smallest n that holds the block and row 1024
    p = CL.posterior_reference(i, n, with_block)
    c = CL.cond2(CL.rung(i, n)[4])
    print("rung %d n %d cond %.1e: LAPACK var %.2e covdiag %.2e invdiag %.2e" % (
        i, n, c, p.err_var_lapack, p.err_covdiag_lapack, p.err_invdiag_lapack))
    assert p.err_var_lapack <= c * n * CL.U and p.err_invdiag_lapack <= c * n * CL.U
    assert np.all(np.asarray(p.var, dtype=float) > -1e-9) and np.all(np.asarray(p.invdiag, dtype=float) > 0.0)
    if with_block:
        print("block: LAPACK %.2e" % p.err_block_lapack)
        assert p.block.shape == (130, 130)
        # K^-1 is symmetric: the refined block is, two digits beyond LAPACK's own error of its entries
        scale = np.abs(p.block).max()
        assert float(np.abs(p.block - p.block.T).max() / scale) <= 1e-2 * float(np.abs(p.block_lapack - p.block).max() / scale)
