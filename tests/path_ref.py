"""Pathwise Thompson draws (Matheron's rule) restated in numpy, fp64 -- the reference of tests/test_path_cpu.py and
tests/test_gpu_path.py.

    f_s(x) = bias + sum_j theta_sj cos(W_sj . x + b_sj)  +  sum_{i < nv} v_si k(x, X_i)
    theta_s = sc w_s,   sc = sqrt(2 rho / n)
    v_s = (K + sn2 I)^-1 r_s,   r_s = (y - bias) - Phi_s(X) theta_s - sqrt(sn2) eps_s

Every evaluation also returns the sum of the ABSOLUTE values of its terms,
    B(x) = |bias| + sum_j |theta_j| + sum_i |v_i| k(x, X_i)
(and the analogous sums of the gradient's terms): the worst-case rounding error of a length-(nv + n) sum in any order is
(nv + n) 2^-53 B, which is what the tolerances below are made of."""
import numpy as np

KERNELS = ('se', 'matern5', 'matern3', 'matern1')
EPS = 2.0 ** -53


def sq_dist(X, Z, ell):
    """r2[i, m] = sum_k ((X_ik - Z_mk) / ell_k)^2 by direct differences of the scaled points."""
    Xs, Zs = np.asarray(X, dtype=float) / ell, np.asarray(Z, dtype=float) / ell
    r2 = np.zeros((len(Xs), len(Zs)))
    for k in range(Xs.shape[1]):
        df = Xs[:, k][:, None] - Zs[:, k][None, :]
        r2 += df * df
    return r2


def kern(kernel, r2, rho):
    """k and g = dk / dr2 (g = 0 at r = 0 for matern1: the kink's gradient is defined as 0, as the device defines it)."""
    if kernel == 'se':
        k = rho * np.exp(-0.5 * r2)
        return k, -0.5 * k
    r = np.sqrt(r2)
    if kernel == 'matern5':
        s = np.sqrt(5.0) * r
        e = np.exp(-s)
        return rho * (1.0 + s + s * s / 3.0) * e, -(5.0 / 6.0) * (1.0 + s) * rho * e
    if kernel == 'matern3':
        s = np.sqrt(3.0) * r
        e = np.exp(-s)
        return rho * (1.0 + s) * e, -1.5 * rho * e
    k = rho * np.exp(-r)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.where(r > 0.0, -0.5 * k / r, 0.0)
    return k, g


def cov(kernel, X, Z, ell, rho):
    return kern(kernel, sq_dist(X, Z, ell), rho)[0]


def features(W, b, X):
    """Phi (S, N, n) = cos(X W_s^T + b_s) for W (S, n, d), b (S, n)."""
    return np.cos(np.einsum('id,snd->sin', np.asarray(X, dtype=float), W) + b[:, None, :])


def weights(kernel, X, y, ell, rho, sn2, bias, W, b, w, eps, sc):
    """theta (S, n), v (S, N), and what the residual bar needs: r (S, N) and Kn = K + sn2 I."""
    X = np.asarray(X, dtype=float)
    S, N = W.shape[0], len(X)
    theta = sc * w
    eps = np.zeros((S, N)) if eps is None else eps
    r = (np.asarray(y, dtype=float) - bias)[None, :] - np.einsum('sin,sn->si', features(W, b, X), theta) - np.sqrt(sn2) * eps
    Kn = cov(kernel, X, X, ell, rho) + sn2 * np.eye(N)
    v = np.linalg.solve(Kn, r.T).T
    return theta, v, r, Kn


def resid_tol(Kn, v, r):
    """The bar tests/test_gpu_configs.py holds alpha to, per draw: 1e-11 (|Kn|_F |v_s| + |r_s|)."""
    return 1e-11 * (np.linalg.norm(Kn) * np.linalg.norm(v, axis=-1) + np.linalg.norm(r, axis=-1))


def values(kernel, Xlead, ell, rho, bias, W, b, theta, v, Xc):
    """f (S, M) and B (S, M); Xlead: the leading nv = v.shape[1] observations."""
    K = cov(kernel, Xlead, Xc, ell, rho)                       # (nv, M)
    prior = np.einsum('smn,sn->sm', features(W, b, Xc), theta)
    f = (bias + prior) + v @ K
    B = abs(bias) + np.abs(theta).sum(1)[:, None] + np.abs(v) @ K
    return f, B


def value_tol(B, f, nv, n, rho):
    """(nv + n + 64) 2^-53 B: any summation order plus a few ulp per covariance; plus the feature part's own bar (rtol 1e-9,
    atol 1e-9 sqrt(rho): tests/test_gpu_configs.py)."""
    return (nv + n + 64) * EPS * B + 1e-9 * np.abs(f) + 1e-9 * np.sqrt(rho)


def value_grad(kernel, Xlead, ell, rho, bias, W, b, theta, v, Xc):
    """ONE draw (W (n, d), b, theta (n,), v (nv,)): f (M,), g (M, d) and the absolute sums Bf (M,), Bg (M, d)."""
    Xc = np.asarray(Xc, dtype=float)
    z = Xc @ W.T + b                                           # (M, n)
    k, gk = kern(kernel, sq_dist(Xlead, Xc, ell), rho)         # (nv, M)
    f = (bias + np.cos(z) @ theta) + v @ k
    Bf = abs(bias) + np.abs(theta).sum() + np.abs(v) @ k
    tg = -(np.sin(z) * theta)[:, :, None] * W[None, :, :]      # (M, n, d): the feature terms of the gradient
    # dk_i / dx_j = g_i 2 (x_j - X_ij) / ell_j^2
    dk = gk.T[:, :, None] * (2.0 * (Xc[:, None, :] - np.asarray(Xlead, dtype=float)[None, :, :]) / (ell * ell))      # (M, nv, d)
    ug = v[None, :, None] * dk
    return f, tg.sum(1) + ug.sum(1), Bf, np.abs(tg).sum(1) + np.abs(ug).sum(1)


def grad_tol(Bg, g, nv, n, rho, ell):
    """The value's form with the gradient's absolute sums; the absolute term in the gradient's units (per length scale)."""
    return (nv + n + 64) * EPS * Bg + 1e-9 * np.abs(g) + 1e-9 * np.sqrt(rho) / ell


def model(N, d, seed, sn2_over_rho, kernel='se'):
    """The models of the GPU tests: X uniform in the unit box, a smooth y, ell = 0.2 + 0.3 u (times sqrt(d / 3) beyond d = 3)."""
    rng = np.random.RandomState(seed)
    X = rng.rand(N, d)
    y = np.sin(3.0 * X.sum(1)) + 0.5 * np.cos(5.0 * X[:, 0]) + 0.1 * rng.randn(N)
    ell = (0.2 + 0.3 * rng.rand(d)) * (np.sqrt(d / 3.0) if d > 3 else 1.0)
    rho = 1.3
    return dict(kernel=kernel, X=X, y=y, ell=ell, rho=rho, sn2=sn2_over_rho * rho, bias=0.2)


def spectral(kernel, n, d, ell, S, seed):
    """S draws of the spectral points and phases as GP.sample_f makes them, and the normals w (S, n)."""
    rng = np.random.RandomState(seed)
    W = rng.randn(S, n, d)
    if kernel != 'se':
        nu = {'matern5': 2.5, 'matern3': 1.5, 'matern1': 0.5}[kernel]
        W = W * np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=(S, n)))[:, :, None]
    W = W / ell
    return W, rng.rand(S, n) * 2.0 * np.pi, rng.randn(S, n)
