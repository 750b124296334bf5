"""CPU-only checks of the Fisher information (include/tgp.h, seam S2j): the two entries against the header and the loaded
library, the chain rule ``kernels.fisher_theta`` against the reference project's own kernel derivatives
(tests/golden/g16_fisher.npz) with F_p from the float64 reference of tests/_fisher_refs.py, the block structure for sums, fixed
hyper-parameters, every refusal of the Python layer with stand-ins for the library, and the two host references against each
other."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import treegp_amd as tg
from treegp_amd import _lib, kernels, ops
from treegp_amd.log_likelihood import log_likelihood

import _fisher_refs as FR
import _ksum_refs as S
import _vk_loglik_grad_refs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_ARBF = "0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))"
GOLDEN_RBF = "0.7**2 * RBF(0.2)"


# ---------------------------------------------------------------------------------------------------------
# the C ABI
def test_entries_match_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "tgp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int (tgp_gp_fisher\w*)\(([^;]*)\);", code, flags=re.M | re.S))
    assert set(protos) == {"tgp_gp_fisher", "tgp_gp_fisher_sum"}
    for name, kernel_t, K in (("tgp_gp_fisher", "tgp_kernel", _lib.TgpKernel), ("tgp_gp_fisher_sum", "tgp_kernel_sum", _lib.TgpKernelSum)):
        args = [" ".join(a.split()) for a in protos[name].split(",")]
        assert args == ["tgp_ctx *ctx", "tgp_factor *f", "const %s *k" % kernel_t, "const double *X", "int64_t n", "double *fisher"]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(K), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert "S2j" in text
    lib = _lib.load_library()
    assert hasattr(lib, "tgp_gp_fisher") and hasattr(lib, "tgp_gp_fisher_sum")


# ---------------------------------------------------------------------------------------------------------
# the chain rule
def golden_case(golden, tag):
    g = golden("g16_fisher.npz")
    kern = str(g[tag + "_kernel"])
    X, _, y_err = V.data_a(200)
    assert np.array_equal(X, g["X"]) and np.array_equal(y_err, g["y_err"])
    return kern, X, y_err, g[tag + "_F"]


@pytest.mark.parametrize("tag", ["arbf", "rbf"])
def test_fisher_theta_against_the_reference_projects_derivatives(golden, tag):
    kern, X, y_err, ref = golden_case(golden, tag)
    assert kern == {"arbf": GOLDEN_ARBF, "rbf": GOLDEN_RBF}[tag]
    k = tg.eval_kernel(kern)
    F_p = FR.fisher_f64(kernels.device_spec(k), X, y_err)
    assert F_p.shape == (4, 4)
    F = kernels.fisher_theta(k, F_p)
    assert F.shape == (len(k.theta), len(k.theta))
    err = FR.rel_err(F, ref)
    print("fisher_theta %s: max rel err against the golden = %.3e" % (tag, err))
    assert err <= 1e-12


def test_block_structure_for_a_sum():
    k = tg.eval_kernel(S.SUM_B)
    leaves = kernels._sum_leaves(k)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((16, 16))
    F_p = A.dot(A.T)
    F = kernels.fisher_theta(k, F_p)
    assert F.shape == (len(k.theta), len(k.theta))
    Js = [kernels.spec_jacobian(leaf, von_karman=True) for leaf in leaves]
    rows = np.cumsum([0] + [len(J) for J in Js])
    assert rows[-1] == len(k.theta)
    for s, Js_ in enumerate(Js):
        for t, Jt in enumerate(Js):
            block = Js_.dot(F_p[4 * s:4 * s + 4, 4 * t:4 * t + 4]).dot(Jt.T)
            np.testing.assert_allclose(F[rows[s]:rows[s + 1], rows[t]:rows[t + 1]], block, rtol=1e-13, atol=1e-13 * np.abs(F).max())
    with pytest.raises(ValueError, match="shape"):
        kernels.fisher_theta(k, F_p[:8, :8])
    with pytest.raises(ValueError, match="shape"):
        kernels.fisher_theta(tg.eval_kernel(GOLDEN_RBF), F_p)


def test_fixed_hyper_parameters_drop_their_rows(golden):
    kern, X, y_err, ref = golden_case(golden, "rbf")
    F_p = FR.fisher_f64(kernels.device_spec(tg.eval_kernel(kern)), X, y_err)
    fixed_amp = tg.eval_kernel("ConstantKernel(0.7**2, constant_value_bounds='fixed') * RBF(0.2)")
    assert len(fixed_amp.theta) == 1
    F = kernels.fisher_theta(fixed_amp, F_p)
    assert F.shape == (1, 1) and abs(F[0, 0] - ref[1, 1]) <= 1e-12 * ref[1, 1]
    fixed_len = tg.eval_kernel("0.7**2 * RBF(0.2, length_scale_bounds='fixed')")
    F = kernels.fisher_theta(fixed_len, F_p)
    assert F.shape == (1, 1) and abs(F[0, 0] - ref[0, 0]) <= 1e-12 * ref[0, 0]
    both = tg.eval_kernel("ConstantKernel(0.7**2, constant_value_bounds='fixed') * RBF(0.2, length_scale_bounds='fixed')")
    assert kernels.fisher_theta(both, F_p).shape == (0, 0)


DENSE_TREES = ["0.7**2 * RBF(0.2) + WhiteKernel(0.01)", "0.7**2 * Matern(0.2, nu=1.5)",
               " + ".join("0.%d**2 * RBF(0.%d)" % (i + 1, i + 1) for i in range(5))]


def test_fisher_theta_refuses_trees_without_a_device_form():
    for kern in DENSE_TREES:
        with pytest.raises(NotImplementedError):
            kernels.fisher_theta(tg.eval_kernel(kern), np.eye(4))


# ---------------------------------------------------------------------------------------------------------
# the Python layer with stand-ins for the library
class FakeFactor(object):
    def __init__(self, n):
        self._h, self._ctx, self.n, self.freed = 1, None, n, []

    def free(self, keep_memory=False):
        self.freed.append(keep_memory)
        self._h = None


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve keeps a FakeFactor, ops.gp_fisher answers with the float64 reference; every call is recorded"""
    calls = []

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        fac = FakeFactor(len(X)) if keep else None
        calls.append(("gp_solve", spec, fac, y_err))
        return (np.zeros(len(X)) if want_alpha else None), 0.0, 0.0, fac

    def gp_fisher(spec, factor, X, ctx=None):
        calls.append(("gp_fisher", spec, factor, None))
        assert factor._h, "the factor was freed before the Fisher call"
        y_err = [c for c in calls if c[0] == "gp_solve"][-1][3]
        return FR.fisher_f64(spec, X, y_err)

    def gp_solve_dense(*a, **k):
        raise AssertionError("the Fisher information has no dense route")

    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_fisher", gp_fisher)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    return calls


def _gp(kern, n=200, nd=2, **kw):
    X, y, y_err = V.data_a(n, nd)
    gp = tg.GPInterpolation(kernel=kern, optimizer="none", **kw)
    gp.initialize(X, y, y_err=y_err)
    return gp


@pytest.mark.parametrize("tag", ["arbf", "rbf"])
def test_object_methods_with_a_stand_in_for_the_device(fake, golden, tag):
    kern, X, y_err, ref = golden_case(golden, tag)
    gp = _gp(kern)
    gp._alpha, gp._factor, gp._factor_key = "alpha", None, "key"
    theta0, kernel0 = np.array(gp.kernel.theta), gp.kernel
    F = gp.return_fisher_information()
    assert FR.rel_err(F, ref) <= 1e-12
    assert [c[0] for c in fake] == ["gp_solve", "gp_fisher"]
    assert fake[0][2] is fake[1][2] and fake[0][2].freed == [True]      # a temporary factor, handed back to the context
    assert gp._alpha == "alpha" and gp._factor is None and gp._factor_key == "key"
    assert gp.kernel is kernel0 and np.array_equal(gp.kernel.theta, theta0)
    cov = gp.return_theta_covariance()
    np.testing.assert_allclose(cov.dot(ref), np.eye(len(ref)), atol=1e-9)
    assert gp._alpha == "alpha" and gp._factor is None and np.array_equal(gp.kernel.theta, theta0)
    # another theta: the object's own stays
    F2 = gp.return_fisher_information(theta=theta0 + 0.1)
    assert F2.shape == F.shape and not np.allclose(F2, F) and np.array_equal(gp.kernel.theta, theta0)
    # the method of the likelihood class gives the same matrix
    F3 = log_likelihood(X, np.zeros(len(X)), y_err).fisher_information(tg.eval_kernel(kern))
    assert np.array_equal(F3, F)


def test_white_noise_is_part_of_the_matrix(fake):
    gp = _gp(GOLDEN_RBF, white_noise=0.3)
    gp.return_fisher_information()
    _, _, y_err = V.data_a(200)
    np.testing.assert_allclose(fake[0][3], np.sqrt(y_err ** 2 + 0.09))


def test_theta_covariance_needs_a_positive_definite_matrix(fake, monkeypatch):
    gp = _gp(GOLDEN_RBF)
    monkeypatch.setattr(ops, "gp_fisher", lambda spec, factor, X, ctx=None: np.diag([1.0, -1.0, 0.0, -1.0]))
    with pytest.raises(np.linalg.LinAlgError):
        gp.return_theta_covariance()

    def not_pd(*a, **k):
        raise np.linalg.LinAlgError("3-th leading minor of the array is not positive definite")
    monkeypatch.setattr(ops, "gp_solve", not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        gp.return_fisher_information()


def test_refusals_of_the_object_methods(fake, monkeypatch):
    X3 = np.random.default_rng(2).uniform(size=(20, 3))
    gp = tg.GPInterpolation(kernel="0.8**2 * RBF([0.2, 0.3, 0.5])", optimizer="none")
    gp.initialize(X3, X3[:, 0], y_err=0.1 * np.ones(20))
    for method in (gp.return_fisher_information, gp.return_theta_covariance):
        with pytest.raises(NotImplementedError, match="3-D"):
            method()
    with pytest.raises(NotImplementedError, match="3-D"):
        log_likelihood(X3, X3[:, 0], 0.1 * np.ones(20)).fisher_information(tg.eval_kernel("0.8**2 * RBF([0.2, 0.3, 0.5])"))
    for kern in DENSE_TREES:
        gp = _gp(kern, n=20)
        for method in (gp.return_fisher_information, gp.return_theta_covariance):
            with pytest.raises(NotImplementedError, match="dense route"):
                method()
        X, y, y_err = V.data_a(20)
        with pytest.raises(NotImplementedError, match="dense route"):
            log_likelihood(X, y, y_err).fisher_information(tg.eval_kernel(kern))
    # an object whose own gate refuses (a sum while the multi-GPU engine would take the problem)
    gp = _gp(S.SUM_A, n=20)

    def refuses(kernel, n=None):
        raise NotImplementedError("sums keep the dense route under the multi-GPU engine")
    monkeypatch.setattr(gp, "_device_spec", refuses)
    with pytest.raises(NotImplementedError, match="multi-GPU engine"):
        gp.return_fisher_information()
    assert fake == []                                              # nothing reached the library


def test_ops_refusals_need_no_device():
    fac = FakeFactor(5)
    with pytest.raises(ValueError, match="KernelSpec3"):
        ops.gp_fisher(ops.KernelSpec3(_lib.TGP_ARBF), fac, np.zeros((5, 3)))
    fac.free()
    with pytest.raises(ValueError, match="freed"):
        ops.gp_fisher(ops.KernelSpec(_lib.TGP_ARBF), fac, np.zeros((5, 2)))
    with pytest.raises(ValueError, match="freed"):
        ops.gp_fisher(ops.KernelSumSpec([ops.KernelSpec(_lib.TGP_ARBF)]), None, np.zeros((5, 2)))


# ---------------------------------------------------------------------------------------------------------
# the references
def test_the_two_host_references_agree():
    X, _, y_err = V.data_a(129)
    for kern in (GOLDEN_ARBF, GOLDEN_RBF, V.SET_A["avk"], V.SET_A["vk"], S.SUM_A):
        spec = kernels.device_spec(tg.eval_kernel(kern))
        F64, Fld = FR.fisher_f64(spec, X, y_err), FR.fisher_longdouble(spec, X, y_err)
        err = FR.rel_err(F64, Fld)
        print("float64 against long double, n = 129, %s: %.3e" % (kern[:28], err))
        assert err <= 1e-12
        assert np.array_equal(F64, F64.T) or FR.rel_err(F64, F64.T) <= 1e-14
    # without noise the amplitude entry is n / 2 (S_0 is the identity)
    for kind in ("avk", "vk"):
        F = FR.fisher_f64(kernels.device_spec(tg.eval_kernel(V.SET_A[kind])), X, None)
        assert abs(F[0, 0] - 64.5) <= 1e-10 * 129
    with pytest.raises(ValueError):
        FR.fisher_longdouble(kernels.device_spec(tg.eval_kernel(GOLDEN_RBF)), np.zeros((FR.LONGDOUBLE_NMAX + 1, 2)), None)
