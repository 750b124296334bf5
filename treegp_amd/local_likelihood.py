"""Maximum-likelihood hyper-parameter search on Vecchia's approximation of the likelihood (not in the reference).

log L ~ sum_i log N(y_i | mu_i, var_i + y_err_i^2), row i conditioned on its k nearest rows among those earlier in a fixed random
ordering (``ops.gp_local_cond(mode="prior")``, seam S3v of include/tgp.h): linear in n, no n x n factor, so a catalogue of
10^5 - 10^6 stars that ``log_likelihood`` cannot factorise still gets a likelihood fit.  The L-BFGS-B driver and its
forward-difference gradient are those of ``log_likelihood``'s non-parallel branch.
"""
import copy

import numpy as np
from scipy import optimize

from . import ops
from . import kernels as _kernels
from ._lib import TgpError
from .kernels import kernel_to_spec
from .log_likelihood import _FD_STEP, _rejects_theta


class local_likelihood(object):
    """:param X: coordinates (n_samples, 1 or 2)  :param y: values  :param y_err: errors
    :param k: neighbours per row, 1 .. 128  :param seed: of the random ordering (``ops.vecchia_rank``)."""

    def __init__(self, X, y, y_err, k=64, seed=0):
        self.X, self.y, self.y_err = X, y, y_err
        self.ndata = len(X[:, 0])
        self.k, self.seed = k, seed
        self.rank = ops.vecchia_rank(self.ndata, seed)
        self._neighbors = None

    def _spec(self, kernel):
        return _kernels.local_spec(kernel, self.X, "optimizer='local-likelihood'", single=kernel_to_spec)

    def find_neighbors(self, kernel):
        """the (n, k) lists of the ordering at ``kernel``'s metric (one search; the values of that call are not used)"""
        try:
            out = ops.gp_local_cond(self._spec(kernel), self.X, self.y, self.y_err, k=self.k, mode="prior", rank=self.rank,
                                    return_neighbors=True)
        except np.linalg.LinAlgError as ex:              # a row failed at the starting kernel: its lists are there all the same
            out = ex.results
        return out[3]

    def log_likelihood(self, kernel, neighbors=None):
        """-1/2 sum (y_i - mu_i)^2 / s2_i - 1/2 sum log s2_i - n/2 log 2 pi; -inf when a row's local matrix is not positive
        definite, as ``log_likelihood.log_likelihood`` gives for K.  ``neighbors``: lists to use instead of a search."""
        spec = self._spec(kernel)
        try:
            _, _, sums = ops.gp_local_cond(spec, self.X, self.y, self.y_err, k=self.k, mode="prior", rank=self.rank,
                                           neighbors=neighbors)
            ll = -0.5 * sums[1] - 0.5 * sums[0] - (0.5 * self.ndata) * np.log(2.0 * np.pi)
        except (np.linalg.LinAlgError, FloatingPointError):
            ll = -np.inf
        except TgpError as ex:
            if "has no Cholesky factor" not in str(ex) and not _rejects_theta(ex):
                raise
            ll = -np.inf
        return float(ll) if np.isfinite(ll) else -np.inf

    def optimizer(self, kernel):
        """L-BFGS-B on -log L_local over theta, gradient by forward differences with ``_FD_STEP``.  The neighbour lists are found
        ONCE, at the starting kernel's metric, and every evaluation is made on them (``neighbors=`` of ``ops.gp_local_cond``):
        the objective is then a smooth function of theta.  Searching again at every theta would make it jump whenever a list
        changes, by more than the differences the gradient is made of.  ``_logL`` is the objective's value at the optimum, on
        those same lists; ``_neighbors`` keeps them."""
        self._spec(kernel)                                # the refusals come before any work
        self._neighbors = self.find_neighbors(kernel)
        work = kernel.clone_with_theta(kernel.theta)

        def cost(theta):
            work.theta = theta
            return -self.log_likelihood(work, neighbors=self._neighbors)

        best = optimize.minimize(cost, kernel.theta, method="L-BFGS-B", options={"eps": _FD_STEP})["x"]
        fitted = kernel.clone_with_theta(best)
        self._kernel = copy.deepcopy(fitted)
        self._logL = self.log_likelihood(self._kernel, neighbors=self._neighbors)
        return fitted
