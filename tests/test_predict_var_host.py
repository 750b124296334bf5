"""CPU-only checks of the posterior-variance seam (S3c): the C-ABI surface and the argument check that runs before any
device work."""
import os
import re

import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgp_gp_predict_var", "tgp_gp_predict_var_dense")


def test_variance_entry_points_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tgp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    for name in NAMES:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), "libtgp.so does not export %s" % name
    # var has one double per query point: the last argument of both is a double array, m the one before it
    assert _lib.SIGNATURES["tgp_gp_predict_var"][1][-2] is _lib._i64
    assert _lib.SIGNATURES["tgp_gp_predict_var_dense"][1][-2] is _lib._i64


@pytest.mark.parametrize("kernel", ["1.0**2 * RBF(0.3)", "0.7**2 * Matern(length_scale=0.3, nu=1.5)"])
def test_cov_and_var_together_are_refused_before_device_work(kernel):
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (16, 2))
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none")
    gp.initialize(X, np.sin(X[:, 0]))
    with pytest.raises(ValueError, match="return_cov and return_var"):
        gp.predict(X, return_cov=True, return_var=True)
    with pytest.raises(ValueError, match="return_cov and return_var"):
        gp.return_gp_predict(gp._residual(), gp._X, X, gp.kernel, gp._y_err, return_cov=True, return_var=True)
    assert gp._alpha is None and gp._factor is None
