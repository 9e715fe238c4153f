"""Helper (not a test): the gradient of the log marginal likelihood in numpy, on oracle.gp_ref.

    Ky = K + sn2 I,  alpha = Ky^-1 (y - bias),  Kinv = Ky^-1,  W = alpha alpha^T - Kinv,  xs = x / ell,  g = dk/dr2
    dL/dsn2   = 1/2 sum_i  W_ii
    dL/drho   = 1/2 sum_ij W_ij k_ij / rho
    dL/dell_k = 1/2 sum_ij W_ij g_ij (-2 (xs_ik - xs_jk)^2 / ell_k)
    dL/dbias  = sum_i alpha_i
in NATURAL parameters [sn2, rho, ell_1..d, bias], and the cancellation-free scales S: the same sums with every term
replaced by its absolute value.  Tolerances of the tests are relative to S, never to the gradient (it vanishes at an
optimum)."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_ref


def loglik_grad(gp):
    """(grad, S) of a fitted GPRef, natural parameters, each of length d + 3."""
    X, ell, rho = gp.X, gp.ell, gp.rho
    n, d = X.shape
    alpha = gp.alpha()
    Linv = sla.solve_triangular(gp.L, np.eye(n), lower=True)
    Kinv = Linv.T @ Linv
    A = np.outer(alpha, alpha)
    W, Wabs = A - Kinv, np.abs(A) + np.abs(Kinv)
    Xs = X / ell
    r2 = gp_ref.sqdist(Xs, Xs)
    k = gp_ref.kern_from_r2(gp.kid, r2, rho)
    g = gp_ref.dkern_dr2(gp.kid, r2, rho)
    grad, S = np.empty(d + 3), np.empty(d + 3)
    grad[0], S[0] = 0.5 * np.trace(W), 0.5 * np.trace(Wabs)
    grad[1], S[1] = 0.5 * np.sum(W * k) / rho, 0.5 * np.sum(Wabs * np.abs(k)) / rho
    for c in range(d):
        df = Xs[:, c][:, None] - Xs[:, c][None, :]
        dK = g * (-2.0 * df * df / ell[c])
        grad[2 + c], S[2 + c] = 0.5 * np.sum(W * dK), 0.5 * np.sum(Wabs * np.abs(dK))
    grad[2 + d], S[2 + d] = np.sum(alpha), np.sum(np.abs(alpha))
    return grad, S


def to_theta(gp, v):
    """A natural-parameter gradient (or scale) in hyper_vector() coordinates [log sn2, log rho, log ell.., bias]."""
    return np.asarray(v) * np.concatenate([[gp.sn2, gp.rho], gp.ell, [1.0]])


class GPRefGrad(gp_ref.GPRef):
    """GPRef whose loglikelihood(grad=True) returns (L, dL/dtheta) in hyper_vector() coordinates."""

    def loglikelihood(self, grad=False):
        L = gp_ref.GPRef.loglikelihood(self)
        if not grad:
            return L
        return L, to_theta(self, loglik_grad(self)[0])

    def copy(self):
        new = GPRefGrad(self.sn2, self.rho, self.ell.copy(), self.bias, self.kid)
        for k, p in self.params.items():
            new.params[k].prior = p.prior
        if self.X is not None:
            new.X, new.Y = self.X.copy(), self.Y.copy()
            new.L, new.a = self.L, self.a
        return new


def init_model_priors(gp, y, bounds):
    """The priors pybo_amd.bayesopt.init_model attaches for observations `y` over `bounds`."""
    from pybo_amd.bayesopt import _heuristic_hypers
    hyp = _heuristic_hypers(y, bounds)
    gp.params['like.sn2'].set_prior('horseshoe', 0.1)
    gp.params['kern.rho'].set_prior('lognormal', np.log(hyp['rho']), 1.0)
    gp.params['kern.ell'].set_prior('uniform', hyp['ell'] / 100, hyp['ell'] * 10)
    gp.params['mean.bias'].set_prior('normal', hyp['bias'], hyp['rho'])
    return gp


# the optimisation problem shared by the CPU and the GPU test: N = 64, d = 2, y drawn from the prior at TRUTH;
# seed chosen on the CPU (of 0..23: L-BFGS-B usually stops on its relative-decrease rule first, with a projected gradient of
# 1e-5..1e-3; at seed 17 the run from truth + 0.5 ends at 1.8e-6, and the start truth + 0.45 reaches the same optimum, 4e-10 apart)
OPT_SEED = 17
OPT_N, OPT_D = 64, 2


def opt_problem(seed=OPT_SEED):
    """(X, y, truth theta, bounds) of the optimisation test."""
    rng = np.random.RandomState(seed)
    bounds = np.array([[0.0, 1.0]] * OPT_D)
    X = rng.rand(OPT_N, OPT_D)
    sn2, rho, ell, bias = 1e-2, 1.0, np.array([0.2, 0.2]), 0.0
    K = gp_ref.kernel(gp_ref.SE_ARD, X, X, ell, rho) + sn2 * np.eye(OPT_N)
    y = bias + np.linalg.cholesky(K) @ rng.randn(OPT_N)
    truth = np.concatenate([[np.log(sn2), np.log(rho)], np.log(ell), [bias]])
    return X, y, truth, bounds
