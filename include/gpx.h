/* gpx.h -- C-ABI of libgpx.so: the MI355X (gfx950) GP-posterior + acquisition engine.
 * The reference (mwhoffman/pybo) has NO native boundary: its GP arithmetic is a set of Python method calls on a duck-typed `model` object (the un-vendored
 * `reggie` package).  Each entry point below therefore cites the *call site in pybo* whose work it performs; pybo_amd/ binds these by ctypes.
 * Conventions
 *   - every function returns an int status: 0 = GPX_OK, negative = error class; gpx_last_error(h) returns a NUL-terminated description (handle-local; NULL
 *     handle -> thread-local string of the last failed gpx_create).
 *   - caller owns every host buffer; arrays are row-major C-contiguous float64 / int64.
 *   - `_dev` variants take DEVICE pointers (e.g. torch.Tensor.data_ptr()) valid on the handle's device; they enqueue on the handle's stream and are synchronous
 *     on return only where an output lands in a host buffer (top-k, status).
 *   - a handle is not re-entrant; distinct handles may be driven from distinct threads.
 *   - a handle owns up to four HIP streams (its own or the caller's + three side streams created on first need); a process that keeps several handles alive
 *     should export GPU_MAX_HW_QUEUES=8 BEFORE its first HIP call, or work meant to overlap inside a handle may share a hardware queue and serialise
 *     (+2.3 ms per warm iteration at N = 8192).  Results never depend on it.
 *   - no C++ exception crosses this boundary.
 */
#ifndef GPX_H
#define GPX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gpx_handle gpx_handle;
enum gpx_status {
    GPX_OK = 0, GPX_EARG = -1, /* bad argument */      GPX_ENOTPD = -2,  /* K + sn2*I not positive definite; see gpx_fail_pivot */
    GPX_EHIP = -3, /* HIP runtime error */   GPX_EOOM = -4, /* device allocation failed */   GPX_ESTATE = -5, /* call order error (e.g. sweep before fit) */
    GPX_ERCCL = -6    /* RCCL could not be loaded, or a collective failed; see gpx_comm_last_error */
};
/* covariance functions; parametrisation (sn2, rho, ell[d], bias) = the arguments of reggie.make_gp(sn2, rho, ell, bias) [pybo/bayesopt.py:98-105] */
enum gpx_kernel {
    GPX_KERN_SE_ARD = 0,   /* rho * exp(-r2/2),                      r2 = sum_k ((x_k-z_k)/ell_k)^2 */
    GPX_KERN_MATERN52 = 1, /* rho * (1 + sqrt5 r + 5 r2/3) exp(-sqrt5 r) */      GPX_KERN_MATERN32 = 2, /* rho * (1 + sqrt3 r) exp(-sqrt3 r) */
    GPX_KERN_MATERN12 = 3  /* rho * exp(-r) */
};
enum gpx_acq {        /* acquisition functions evaluated by the sweep */
    GPX_ACQ_EI = 0,   /* model.get_improvement(target, X)  [pybo/policies/simple.py:25]  params = {target} */
    GPX_ACQ_PI = 1,   /* model.get_tail(target, X)         [pybo/policies/simple.py:39]  params = {target} */
    GPX_ACQ_UCB = 2,  /* mu + sqrt(beta*s2)                [pybo/policies/simple.py:62-73] params = {beta} */
    GPX_ACQ_MEAN = 3, /* posterior mean                    [pybo/recommenders.py:19-25]  no params */
    GPX_ACQ_MES = 16, /* max-value entropy search: mean_s g((y*_s - mu) / sqrt(s2)), g(c) = c phi(c) / (2 Phi(c)) - log Phi(c); ids 4 .. 15: refused.
                       * params = the S sampled maxima y*_s, 1 <= nparams = S <= 64, all finite (else GPX_EARG); gpx_ensemble_sweep*: n_members * S of them,
                       * member-major, member m scores with its slice.  Taken by gpx_sweep*, gpx_sweep_update*, gpx_ensemble_sweep*; never pruned; no batch. */
    GPX_ACQ_KG = 32   /* knowledge gradient over a support set A (Frazier 2009): E_Z max(mu(z) + b_0 Z, max_j mu(a_j) + b_j Z) - max(mu(z), max_j mu(a_j)),
                       * b_0 = s2 / D, b_j = Sigma(a_j, z) / D, D = sqrt(s2 + sn2).  params = A, raw coordinates (m, d) row-major on the HOST, nparams = m d,
                       * 1 <= m <= 127, finite (else GPX_EARG).  Taken by gpx_sweep* ONLY (every output, cache seeding); never pruned.  Ids 17 .. 31: refused */
};
/* ---- lifetime --------------------------------------------------------------------------- */
/* `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for a library-owned stream. */
int gpx_create(int device, void *stream, gpx_handle **out);
int gpx_destroy(gpx_handle *h);      const char *gpx_last_error(const gpx_handle *h);
int gpx_version(void);
/* Options (int64 values), defaults in brackets: schedules that give BIT-IDENTICAL results unless an option says otherwise.  Measurements: DESIGN.md section 4.
 *   "chunk"          candidate columns per sweep chunk, a multiple of 128 [by size: 65536; 131072 up to N = 4096]
 *   "tile_order"     sweep-kernel schedule: bits 0-1 blockIdx->tile map (0 linear heavy-first, 1 per-XCD candidate slices, 2 per-XCD 8x8 super-tiles, 3 the
 *                    same with every workgroup computing the PAIR of tiles (nP-1-i, nt), (i, nt): equal work), bits 2-4 k-loop (4 = operands by LDS-DMA,
 *                    k-step 32, two workgroups per CU, the all-zero quarter-rows of T's diagonal block skipped; 3 = the same without the skip; 1 =
 *                    barrier-free, every wave fetching its own operand halves; 7 = k-step 16, three workgroups per CU; 6 / 5 / 2 = the register-staged loops
 *                    of rounds 5 / 2 / 1: independently scheduled witnesses) [-1 = by size: 7 below 32 block rows, else 19]
 *   "super_m"        rows of the XCD super-tile of 64 workgroups: 1, 2, 4, 8, 16 [8];  "sweep_cols": candidates per tile of k-loop 4: 128, 64, 32 [-1: by size]
 *   "sweep_images"   LDS images of k-loop 4: 1 (two workgroups per CU), 2 (one per CU, the next k-step loads meanwhile) [-1: 2 where no CU would hold two]
 *   "sweep_cache"    1: full sweeps keep candidates and reduced sums for gpx_sweep_update; 0: leave a live cache alone; -1: drop it [0]
 *   "prune"          EI sweeps for ONLY the top-k (ensembles: members[0]'s value) skip what a bound rules out: -1 by size and gate, 0 never, 1 where legal [-1]
 *                    (-1: a sweep whose pruning paid lets the next of the same shape skip the gate: kept across fits / appends, dropped by ANY gpx_set_option)
 *   "eager_inverse"  1: form the triangular inverse inside gpx_fit instead of on first use [0]
 *   "trtri_ahead"    1: when the inverse is certain or likely to follow a fit, its part that needs only the factor's leading block
 *                    rows runs on a side stream behind the factorisation's tail, from "trtri_ahead_min" (8) blocks on [1]
 *   "trtri_left"     1: T21 = -(T22 L21) T11 instead of -T22 (L21 T11); agrees to rounding, NOT bit for bit [0]
 *   "refine_inverse" 1: one Newton step on the inverse, T <- (2I - T R^T) T (squares the left residual; for cond(K) >~ 1e9) [0]
 *   "grad_form"      gpx_predict WITH gradients: 0 auto (one point: one pass over T with 1 + d right-hand sides; batches: two
 *                    passes), 1 always two passes, 2 always one; the forms agree to rounding [0]
 *   "grad_kernel"    triangular matvec of the two-pass form: -1 auto, 0 one wave per row, 1 register-blocked [-1]
 *   "chol_tg"        1: the factorisation is ONE persistent task-graph kernel for fits of "chol_tg_min" (2) .. "chol_tg_max" (160) 128-blocks; 0: the stream
 *                    schedule (~250 launches over four streams) [1].  "chol_tg_db" -1 / 0 / 1: one workgroup per CU with two k-step images of LDS up to
 *                    "chol_tg_db_max" (112) blocks / never / always [-1]; "chol_tg_fuse" 1: a column's solve and the final chunk of the tile below it are one
 *                    task [1]; "chol_tg_tmo_ms": bound of every spin -- on expiry the fit re-runs on the stream schedule and says so on stderr [2000]
 *   "chol_w", "chol_rl", "chol_merge", "chol_fuse", "chol_graph"   the stream schedule: outer panel width in blocks (2..8, 0 = by size), right- / left-looking
 *                    in-panel updates [1], far updates of two panels in one pass [1], diagonal block factored in the panel solve [0], replay from hipGraph [0]
 * Diagnostic knobs ("chol_tg_chunks", "chol_tg_nap", "chol_tg_grid", "chol_tg_isolate", "chol_tg_trace", "grad_rb_cs", "x_rff", "x_bg*", "x_skip" -- the last
 * one leaves parts of the factorisation OUT) exist only in a library built with -DGPX_DIAGNOSTICS (pybo_amd/csrc/libgpx_diag.so; pybo_amd/csrc/gpx_diag.h); the
 * shipping library answers them with GPX_EARG. Environment: GPX_OPTIONS="name=value,name=value" applies options to every handle at creation (A/B runs through a
 * plug-in layer whose handles the caller never sees); a bad entry fails gpx_create with GPX_EARG. */
int gpx_set_option(gpx_handle *h, const char *name, int64_t value);
/* ---- GP fit = model.add_data(X, Y)            [pybo/bayesopt.py:114,258,269] ------------- */
/* Limits: 1 <= d <= 1024 for every entry point (the Thompson / RFF kernels keep a whole feature tile in LDS up to d = 64 and walk the coordinates 32 at a
 * time beyond); top-k requests k <= 4096 (64 per pass over the values).  Gram build K = k(X,X) + sn2 I and Cholesky K = R^T R.  The triangular inverse
 * T = R^-T, a = T (y - bias) and alpha follow on FIRST USE (sweep, predict, mean_at_obs, loglik, append, introspection): the Thompson entry points never
 * read them.  X is (N,d), y is (N,), ell is (d,) on the HOST in both variants. */
int gpx_fit(gpx_handle *h, const double *X, int64_t N, int64_t d, const double *y, int kernel_id, const double *ell, double rho, double sn2, double bias);
int gpx_fit_dev(gpx_handle *h, const double *dX, int64_t N, int64_t d, const double *dy, int kernel_id, const double *ell, double rho, double sn2, double bias);
/* log marginal likelihood of the fit, -1/2 a.a - sum log R_ii - N/2 log 2pi: what reggie.MCMC [pybo/bayesopt.py:115] evaluates once per proposal */
int gpx_loglik(gpx_handle *h, double *out);
/* The same for B hyper-parameter vectors at once on the handle's RESIDENT data, without touching the handle's own fit: hypers (B, d + 3) row-major [sn2, rho,
 * ell_1..d, bias] (the argument order of reggie.make_gp, pybo/bayesopt.py:105), out (B,); -inf where K + sn2 I is not positive definite.  One batched launch
 * chain and one host synchronisation per 64 vectors: what reggie.MCMC(model, n=10, burn=100) [pybo/bayesopt.py:115] repeats per proposal. */
int gpx_loglik_batch(gpx_handle *h, int64_t B, const double *hypers, double *out);
/* L = gpx_loglik (loglik may be NULL) and its gradient, grad (d + 3), in the order [sn2, rho, ell_1..d, bias] of gpx_loglik_batch's rows
 * (natural parameters): what maximum-likelihood / MAP fitting of the hyper-parameters asks for.  From the fitted handle's T, alpha and
 * scaled inputs: N^3/3 multiply-adds on the tile engine, one host synchronisation, no atomics (same fit, same bits); fit and sweep cache untouched. */
int gpx_loglik_grad(gpx_handle *h, double *loglik, double *grad);
/* Incremental fit: absorb ONE more observation x (d,), y into the current factorisation in O(N^2) (two memory-bound passes over T and U) instead of refitting
 * -- the per-iteration `model.add_data(x, y)` of the BO loop [pybo/bayesopt.py:269].  A full 128-block is extended inside buffers allocated with head-room
 * (device copy, no refit).  GPX_ENOTPD like gpx_fit.  A live sweep cache (below) is corrected for the new observation in the same call (one N*M pass). */
int gpx_append(gpx_handle *h, const double *x, double y);
/* ANNOUNCE the next observation's location before its value exists (between `x, _ = solver(index, bounds)` and `y = objective(x)`, pybo/bayesopt.py:265-268:
 * the time the reference spends idle): everything of the coming gpx_append(h, x, y) that does not depend on y is enqueued now without a host synchronisation --
 * k(X, x), the two triangular passes and, on a side stream, the N*M covariance evaluations of the sweep-cache correction.  A following gpx_append with the
 * bit-identical x then costs O(N + M); any other x, or a model change, and the announcement is ignored.  Results bit-identical to an unannounced append.
 * GPX_ESTATE (nothing started, not an error) without a live sweep cache or when the next append has to add a 128-block first. */
int gpx_append_begin(gpx_handle *h, const double *x);
int64_t gpx_fail_pivot(const gpx_handle *h);     /* 0-based index of the failing pivot of the last GPX_ENOTPD fit, else -1. */
/* introspection for parity tests (host outputs): which = 0: L (N,N) lower Cholesky factor, row-major (K + sn2 I = L L^T);
 * 1: T = L^-1 (N,N) lower; 2: K + sn2 I, upper triangle (only after gpx_fit_stage(.., 1): the factorisation consumes it) */
int gpx_get_matrix(gpx_handle *h, int which, double *out);
/* a = L^-1 (y - bias), alpha = (K + sn2 I)^-1 (y - bias), both (N,); gpx_fit_stage (parity): the fit, stopped after the Gram build (stage 1) or Cholesky (2) */
int gpx_get_vectors(gpx_handle *h, double *a, double *alpha);
int gpx_fit_stage(gpx_handle *h, const double *X, int64_t N, int64_t d, const double *y,
                  int kernel_id, const double *ell, double rho, double sn2, double bias, int stage);
/* posterior (latent) mean at the N observed points, closed form y - sn2*alpha = model.predict(X_obs)[0] [pybo/policies/simple.py:21,35] */
int gpx_mean_at_obs(gpx_handle *h, double *mu_host, double *mu_max);
/* posterior (latent) variance at the N observed points, closed form sn2 - sn2^2 [K^-1]_ii with [K^-1]_ii = sum_m U[i][m]^2 (one HBM-read pass over
 * U = R^-1; a sweep over X_obs is an N x N x N product) = model.predict(X_obs)[1] [pybo/policies/simple.py:21,35; pybo/recommenders.py:34] */
int gpx_var_at_obs(gpx_handle *h, double *s2_host);
/* rows (a multiple of 128) the factor buffers are allocated for: 4 matrices of capacity^2 doubles stay on the device until gpx_destroy (size pools by it) */
int64_t gpx_capacity(const gpx_handle *h);
/* ---- posterior moments = model.predict(X, grad) [pybo/policies/simple.py:64] ------------- */
/* Xc (M,d) -> mu, s2 (M,) latent variance; dmu, ds2 (M,d) optional (NULL).  With gradients M = 1 takes the one-pass form, batches the two-pass: "grad_form". */
int gpx_predict(gpx_handle *h, const double *Xc, int64_t M, double *mu, double *s2, double *dmu, double *ds2);
/* The mean alone, mu (M,) and optionally dmu (M,d) (NULL to skip): mu = bias + k(x, X).alpha reads neither the factor nor its inverse -- what the latent
 * recommender maximises, model.predict(X, True)[0::2] [pybo/recommenders.py:17-24], without the two triangular passes per point the variance costs. */
int gpx_predict_mean(gpx_handle *h, const double *Xc, int64_t M, double *mu, double *dmu);
/* The JOINT latent posterior at M points, 1 <= M <= 4096, all buffers on the host -- the reference's demos call model.sample(X, ...).  mu (M,)
 * optional; cov (M,M) row-major, the FULL matrix k(Z,Z) - V^T V with V = T k(X,Z): raw (no clamp on the diagonal), symmetric bit for bit.  Both
 * calls: one host synchronisation; the fit, a live sweep cache, queued corrections and a pending gpx_append_begin are left as they are. */
int gpx_predict_cov(gpx_handle *h, const double *Xc, int64_t M, double *mu, double *cov);
/* S joint draws from the caller's standard normals z (S,M): out (S,M), out[s] = mu + R^T z[s], R^T R = cov + (noisy ? sn2 : 0) I + jitter I (R upper;
 * jitter finite, >= 0).  A draw's bits do not depend on S.  GPX_ENOTPD (out undefined): gpx_last_error names the pivot; gpx_fail_pivot still describes fits. */
int gpx_sample_joint(gpx_handle *h, const double *Xc, int64_t M, const double *z, int64_t S, int noisy, double jitter, double *out);
/* ---- acquisition sweep + top-k = the solver's batched index call and argsort: finit = f(xgrid); idx = argsort(finit)[::-1] [pybo/solvers/lbfgs.py:50-51] */
/* Evaluates acq over M candidates, returns the k best (value desc, then index asc) in host buffers top_val[k], top_idx[k] (indices are LOCAL to Xc;
 * add your shard offset).  acq_all, mu, s2 (each (M,), host in gpx_sweep / device in gpx_sweep_dev) are optional (NULL to skip). */
int gpx_sweep(gpx_handle *h, int acq_id, const double *params, int nparams, const double *Xc, int64_t M, int64_t k,
              double *top_val, int64_t *top_idx, double *acq_all, double *mu, double *s2);
int gpx_sweep_dev(gpx_handle *h, int acq_id, const double *params, int nparams, const double *dXc, int64_t M, int64_t k,
                  double *top_val, int64_t *top_idx, double *d_acq_all, double *d_mu, double *d_s2);
/* ---- warm BO step: the NEXT iteration's `index(xgrid)` over the SAME grid with the SAME hyper-parameters [pybo/bayesopt.py:262-269 with a fixed `xgrid=` in
 *      pybo/solvers/lbfgs.py:42-50].  The reference pays a full refit and a full solve again; with option "sweep_cache" = 1 a full gpx_sweep* keeps the
 *      candidates and their reduced sums q = colsum(V^2), p = V^T a in HBM (8 (d + 2) M bytes), every gpx_append adds the one new row of V to them (N*M
 *      covariance evaluations; up to 8 appended points share one pass), and gpx_sweep_update re-scores the whole grid in O(M) (the target / beta may change
 *      from call to call) + top-k.  Outputs as in gpx_sweep*.  GPX_ESTATE without a valid cache (never swept, or refitted since). */
int gpx_sweep_update(gpx_handle *h, int acq_id, const double *params, int nparams, int64_t k, double *top_val,
                     int64_t *top_idx, double *acq_all, double *mu, double *s2);
int gpx_sweep_update_dev(gpx_handle *h, int acq_id, const double *params, int nparams, int64_t k,
                         double *top_val, int64_t *top_idx, double *d_acq_all, double *d_mu, double *d_s2);
/* nb greedy picks on the LIVE sweep cache, each conditioned on the ones before it at their posterior mean (mean fixed, variance shrinks).
 * EI / PI / UCB (GPX_ACQ_MEAN: GPX_EARG).  1 <= nb <= min(64, M).  sel_val, sel_idx (nb) required; sel_s2 (nb) and s2all (M: the variances
 * that scored the LAST pick) optional, all host.  Model, cache, queued corrections and a pending announcement are untouched. GPX_ESTATE without a cache. */
int gpx_sweep_batch(gpx_handle *h, int acq_id, const double *params, int nparams, int64_t nb, double *sel_val, int64_t *sel_idx, double *sel_s2, double *s2all);
/* The same with the pending outcomes INTEGRATED OUT over S joint fantasies (Snoek et al. 2012).  EI / PI only (else GPX_EARG): value = mean_s acq(mu +
 * sum_{l<j} v_l eps[s][l], s2, t_s), eps (S, ld_eps >= max(nb - 1, 1)) finite standard normals, 1 <= S <= 64.  incumbent 0: t_s = params[0]; 1: t_s <- max(t_s,
 * fantasy s's mean at each pick after its observation).  Rounds < npend < nb: forced to the distinct rows pend_idx.  S = 1, eps = 0: gpx_sweep_batch's bits. */
int gpx_sweep_batch_fantasy(gpx_handle *h, int acq_id, const double *params, int nparams, int64_t nb, const double *eps, int64_t S, int64_t ld_eps,
                            int incumbent, const int64_t *pend_idx, int64_t npend, double *sel_val, int64_t *sel_idx, double *sel_s2, double *s2all);
/* Knowledge gradient (GPX_ACQ_KG) and its gradient at M <= 4096 points, host buffers: A (m, d) the support set as for the sweep, f (M,), g (M, d) -- the
 * `f(x, grad=True)` of the L-BFGS refinement.  f agrees with the sweep's value to rounding.  One host synchronisation; fit, sweep cache and queue untouched. */
int gpx_kg_grad(gpx_handle *h, const double *A, int64_t m, const double *Xc, int64_t M, double *f, double *g);
int64_t gpx_sweep_cache_size(const gpx_handle *h);     /* number of candidates in the live sweep cache (0: none) */
/* ---- Thompson sampling = model.sample_f(n, rng).get(X)   [pybo/policies/simple.py:44-48] -- */
/* S random-Fourier-feature posterior draws f_s(x) = bias + sum_j theta[s][j] cos(W[s][j].x + b[s][j]) (the sqrt(2 rho/n) factor is folded into theta by the
 * caller).  W (S,n,d), b (S,n), theta (S,n) on the host.  Per draw returns the k best candidates: top_val (S,k), top_idx (S,k).  vals_all (S,M) optional. */
int gpx_rff_sweep(gpx_handle *h, const double *W, const double *b, const double *theta, int64_t S, int64_t n, int64_t d, double bias,
                  const double *Xc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *vals_all);
int gpx_rff_sweep_dev(gpx_handle *h, const double *W, const double *b, const double *theta, int64_t S, int64_t n, int64_t d, double bias,
                      const double *dXc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *d_vals_all);
/* value f (M,) and gradient g (M,d) of ONE draw at M points (host buffers): `f(x[None], grad=True)` of the L-BFGS refinement [pybo/solvers/lbfgs.py:56-58] */
int gpx_rff_grad(gpx_handle *h, const double *W, const double *b, const double *theta, int64_t n,
                 int64_t d, double bias, const double *Xc, int64_t M, double *f, double *g);
/* feature Gram for the weight posterior: Phi = cos(X_obs W^T + b) (N,n) on the device's X_obs; host outputs A = Phi^T Phi (n,n), v = Phi^T (y - bias) (n,) */
int gpx_rff_gram(gpx_handle *h, const double *W, const double *b, int64_t n, double *A, double *v);
/* the same for S draws in one call: W (S,n,d), b (S,n) -> A (S,n,n), v (S,n) */
int gpx_rff_gram_batch(gpx_handle *h, const double *W, const double *b, int64_t S, int64_t n, double *A, double *v);
/* the weight posterior of S draws WITHOUT leaving the device (the n x n solve inside sample_f, pybo/policies/simple.py:48): feature Grams as above, then per
 * draw  B = sc^2 A + sn2 I = L L^T,  theta = sc ( B^-1 (sc v) + sqrt(sn2) L^-T z )  with z (S,n) the caller's standard-normal draws, sc = sqrt(2 rho / n) and
 * sn2 the fitted noise variance (> 0); theta (S,n) comes back ready for gpx_rff_sweep* / gpx_rff_grad.  n <= 127: all S draws in one launch chain (the n x n
 * posterior of a draw lives in LDS); 128 <= n <= 4096: per draw the blocked Cholesky kernels of the fit + two vector substitutions (`n` is a free keyword
 * of the reference's sample_f, pybo/policies/simple.py:44).  GPX_ENOTPD if a B is not PD. */
int gpx_rff_posterior(gpx_handle *h, const double *W, const double *b, const double *z, int64_t S, int64_t n, double sc, double *theta);
/* ---- pathwise Thompson draws (Matheron's rule; Wilson et al. 2020): f_s(x) = bias + sum_j theta_sj cos(W_sj.x + b_sj) + sum_{i<nv} v_si k(x, X_i): the RFF
 *      draw is the PRIOR, corrected exactly by the factorisation.  FITTED handle (else GPX_ESTATE); W, b as gpx_rff_*; d the handle's, 1 <= n <= 4096.
 * gpx_path_weights: theta (S,n) = sc*w; v (S,N) = (K + sn2 I)^-1 ((y - bias) - Phi_s(X) theta_s - sqrt(sn2) eps_s); w (S,n), eps (S,N) the caller's standard
 *      normals (eps == NULL: zeros); host buffers.  Forms the inverse on first use.  One host synchronisation; the fit, a live sweep cache, queued
 *      corrections and a pending gpx_append_begin are left as they are.
 * gpx_path_sweep*: f_s over M candidates + per-draw top-k, outputs exactly as gpx_rff_sweep*, time in slot [7]; v (S,nv), 1 <= nv <= N: conditioned on the
 *      handle's LEADING nv observations (a handle appended to since still evaluates the same function; the hyper-parameters are the caller's to keep fixed).
 * gpx_path_grad: value f (M,) and gradient g (M,d) of ONE draw at M <= 4096 points, host buffers; f agrees with the sweep's value to rounding. */
int gpx_path_weights(gpx_handle *h, const double *W, const double *b, const double *w, const double *eps, int64_t S, int64_t n, double sc,
                     double *theta, double *v);
int gpx_path_sweep(gpx_handle *h, const double *W, const double *b, const double *theta, const double *v, int64_t nv, int64_t S, int64_t n, int64_t d,
                   double bias, const double *Xc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *vals_all);
int gpx_path_sweep_dev(gpx_handle *h, const double *W, const double *b, const double *theta, const double *v, int64_t nv, int64_t S, int64_t n, int64_t d,
                       double bias, const double *dXc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *d_vals_all);
int gpx_path_grad(gpx_handle *h, const double *W, const double *b, const double *theta, const double *v, int64_t nv, int64_t n, int64_t d, double bias,
                  const double *Xc, int64_t M, double *f, double *g);
/* ---- hyper-parameter ensemble = pybo's DEFAULT model, reggie.MCMC(gp, n=10) [pybo/bayesopt.py:115]: every index is the average over the n member
 *      GPs.  `members` are fitted handles on ONE device with the same input dimension (members[0] owns the scratch and the error text).
 *      EI / PI: value = mean_m acq_m(x).  UCB / MEAN: mixture moments mu = mean_m mu_m, s2 = mean_m(s2_m + mu_m^2) - mu^2, value = mu + sqrt(params[0] * s2)
 *      (UCB) or mu (MEAN); only these two can return mu / s2.  The member sweeps never leave the device; sums run in member order and are divided once
 *      by n.  Outputs as in gpx_sweep / gpx_sweep_dev; an EI call for the top-k alone prunes as they do ("prune" of members[0]). */
int gpx_ensemble_sweep(gpx_handle *const *members, int n_members, int acq_id, const double *params, int nparams, const double *Xc,
                       int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *acq_all, double *mu, double *s2);
int gpx_ensemble_sweep_dev(gpx_handle *const *members, int n_members, int acq_id, const double *params, int nparams, const double *dXc,
                           int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *d_acq_all, double *d_mu, double *d_s2);
/* gpx_sweep_batch on the ensemble: nb greedy picks scored by the rule above, the members FROZEN (1 <= n_members <= 64, each handle once), every member
 * conditioned on a pick at its own posterior mean.  Every member holds a live sweep cache of the same candidates (none: GPX_ESTATE; other sizes or
 * rows: GPX_EARG, outputs undefined).  sel_val, sel_idx (nb) required; sel_s2 (n_members, nb) optional: the member's conditioned variance at its pick. */
int gpx_ensemble_sweep_batch(gpx_handle *const *members, int n_members, int acq_id, const double *params, int nparams, int64_t nb,
                             double *sel_val, int64_t *sel_idx, double *sel_s2);
/* per-member posterior moments AND gradients at M points (host buffers), member-major: mu, s2 (n_members, M); dmu, ds2 (n_members, M, d) -- the
 * `f(x, grad=True)` calls of the L-BFGS refinement on the default model [pybo/solvers/lbfgs.py:56-58 over pybo/bayesopt.py:115]; the members'
 * latency-bound kernels run concurrently on their own streams (one call instead of n_members gpx_predict calls) and the caller forms the average it
 * needs (mixture moments for UCB / mean, the mean of the members' EI / PI and their gradients). */
int gpx_ensemble_predict(gpx_handle *const *members, int n_members, const double *Xc, int64_t M, double *mu, double *s2, double *dmu, double *ds2);
/* ---- constrained optimisation: cEI(x) = acq_f(x) * prod_j Pr(c_j(x) >= thr[j]) (Gardner et al. 2014; Gelbart et al. 2014): one fitted handle for the
 *      objective and one per black-box constraint, 1 <= nc <= 16, each with its own hyper-parameters, on ONE device with the same d, every handle once (else
 *      GPX_EARG; unfitted: GPX_ESTATE).  With obj, acq_id is GPX_ACQ_EI or GPX_ACQ_PI (non-negative values; others GPX_EARG); obj = NULL (no feasible
 *      incumbent yet): the value is the probability of feasibility alone, acq_id / params are not read.  The lead (obj, else cons[0]) owns the scratch and
 *      the error text.  thr (nc,) finite.  Per candidate v_0 = acq, v_j = v_{j-1} * min(P_j, 1) in the caller's order, P_j the bits of gpx_sweep(GPX_ACQ_PI,
 *      {thr[j]}) on cons[j]; pof_all (optional, (M,)): the same product started at 1; acq_all optional; top-k and `_dev` as gpx_sweep*.  An EI call for the
 *      top-k alone skips what the OBJECTIVE's bound rules out ("prune" of obj; never with a "sweep_cache" on): constraints sweep seeds and survivors only. */
int gpx_constrained_sweep(gpx_handle *obj, gpx_handle *const *cons, int nc, const double *thr, int acq_id, const double *params, int nparams,
                          const double *Xc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *acq_all, double *pof_all);
int gpx_constrained_sweep_dev(gpx_handle *obj, gpx_handle *const *cons, int nc, const double *thr, int acq_id, const double *params, int nparams,
                              const double *dXc, int64_t M, int64_t k, double *top_val, int64_t *top_idx, double *d_acq_all, double *d_pof_all);
/* gpx_ensemble_sweep_batch's rules (live caches of the same candidates, 1 <= nb <= min(64, M), handles untouched) on this index: nb greedy picks, target and
 * thr frozen, the objective and every constraint conditioned on a pick at ITS OWN posterior mean.  Arguments as above; sel_s2 (members, nb) optional. */
int gpx_constrained_sweep_batch(gpx_handle *obj, gpx_handle *const *cons, int nc, const double *thr, int acq_id, const double *params, int nparams,
                                int64_t nb, double *sel_val, int64_t *sel_idx, double *sel_s2);
/* ---- two objectives, maximised: expected hypervolume improvement (Emmerich et al. 2011; Yang et al. 2019) of independent posteriors over the front of the raw
 *      points P (np, 2), 0 <= np <= 4096, above the reference point ref (2); P, ref finite, on the HOST in every variant.  Points not strictly above ref,
 *      weakly dominated ones and duplicates are dropped; at most 1024 may remain (else GPX_EARG); np = 0: an empty front.  With the n survivors by f1
 *      ascending, a_0 = ref[0], a_i = f1_i, b_i = f2_{i+1}, b_n = ref[1]: value = sum_{i=0..n} max(EI_1(a_i) - EI_1(a_{i+1}), 0) EI_2(b_i), EI_1(a_{n+1}) := 0,
 *      EI_j(t) the bits of gpx_sweep(GPX_ACQ_EI, {t}) on f_j; from +0.0, in strip order, every product rounded.  f1 != f2 fitted (GPX_ESTATE) on ONE device,
 *      same d; f1 (the lead) owns scratch, error text and top-k pairs.  Never pruned; a member's live sweep cache: as gpx_sweep_dev of it.  acq_all optional;
 *      d_mom (optional, (4, M) device): mu1, s2_1, mu2, s2_2 as the fold read them.  gpx_ehvi_fold_dev: the fold + top-k alone on the caller's moments (e.g.
 *      of two gpx_sweep_update_dev), on lead's stream. */
int gpx_ehvi_sweep(gpx_handle *f1, gpx_handle *f2, const double *P, int np, const double *ref, const double *Xc, int64_t M, int64_t k,
                   double *top_val, int64_t *top_idx, double *acq_all);
int gpx_ehvi_sweep_dev(gpx_handle *f1, gpx_handle *f2, const double *P, int np, const double *ref, const double *dXc, int64_t M, int64_t k,
                       double *top_val, int64_t *top_idx, double *d_acq_all, double *d_mom);
int gpx_ehvi_fold_dev(gpx_handle *lead, const double *d_mom, int64_t M, const double *P, int np, const double *ref, int64_t k,
                      double *top_val, int64_t *top_idx, double *d_acq_all);
/* gpx_ensemble_sweep_batch's rules on this index: nb greedy picks, f1, f2 and ref frozen, each conditioned on a pick at ITS OWN posterior mean, and the pick's
 * believed outcome (mu_1, mu_2) taken into the front before the next round (on the device; n + nb - 1 <= 1024, else GPX_EARG).  Optional, on the host:
 * sel_s2 (2, nb), sel_y (nb, 2) the believed outcomes, sel_nfront (nb) the size of the front that scored pick j. */
int gpx_ehvi_sweep_batch(gpx_handle *f1, gpx_handle *f2, const double *P, int np, const double *ref, int64_t nb,
                         double *sel_val, int64_t *sel_idx, double *sel_s2, double *sel_y, int64_t *sel_nfront);
/* ---- candidate grid generated and kept in HBM = the solver's grid xgrid = init_uniform(bounds, ngrid, rng) [pybo/solvers/lbfgs.py:45;
 *      pybo/inits/methods.py:24-38] or a Sobol' grid [pybo/inits/methods.py:62-77] without the host array and its PCIe upload; pass gpx_grid_data() to
 *      the *_dev sweeps.
 * GPX_GRID_UNIFORM: counter-based Philox4x32-10, key = seed, counter = element-pair index; element 2c, 2c+1 of the row-major (first+M,d) array = the two
 *      53-bit uniforms of output c; x = lo + u*(hi-lo); rows first .. first+M-1 of that array are generated (a shard holds the numbers the whole grid holds).
 * GPX_GRID_SOBOL: unscrambled Sobol' points first .. first+M-1 in Gray-code order (the order of scipy.stats.qmc.Sobol), from caller-supplied direction
 *      numbers sv (d, bits) uint32, 1 <= bits <= 32.  bounds (d,2) row-major [lo, hi].  Errors of the grid calls are read with gpx_last_error(NULL). */
typedef struct gpx_grid gpx_grid;      enum { GPX_GRID_UNIFORM = 0, GPX_GRID_SOBOL = 1 };
int gpx_grid_create(int device, int kind, const double *bounds, int64_t M, int64_t d, uint64_t seed,
                    int64_t first, const uint32_t *sv, int bits, gpx_grid **out);
const double *gpx_grid_data(const gpx_grid *g);     /* device pointer, (M,d) row-major */
int gpx_grid_rows(gpx_grid *g, const int64_t *idx, int64_t k, double *out);     /* rows idx[0..k) -> out (k,d) host; idx == NULL: the whole grid (M,d) */
int gpx_grid_destroy(gpx_grid *g);
/* ---- multi-GPU exchange: the one collective of the sharded sweep.  The reference is single-process (its only hint at parallelism is the comment
 *      pybo/solvers/lbfgs.py:60); layout per SURVEY.md 8(e): one process per GPU, candidates sharded contiguously, every rank fits redundantly
 *      (bitwise-identical factor), each rank's best (value, GLOBAL index) pairs all-gathered over RCCL/xGMI and merged "value descending, then index
 *      ascending".  RCCL is bound at run time (dlopen of librccl, override with $GPX_RCCL_LIB): single-GPU use never loads it.  Errors: gpx_comm_last_error */
typedef struct gpx_comm gpx_comm;
#define GPX_COMM_ID_BYTES 128
int gpx_comm_unique_id(unsigned char *id);     /* rank 0 generates the id (ncclGetUniqueId) and hands its 128 bytes to every rank over any side channel */
/* collective over all ranks: binds the communicator to the handle's device and stream */
int gpx_comm_init(gpx_handle *h, int rank, int nranks, const unsigned char *id, gpx_comm **out);
int gpx_comm_destroy(gpx_comm *c);
int gpx_comm_size(const gpx_comm *c, int *rank, int *nranks);
const char *gpx_comm_last_error(void);
/* All-gather of the n (value, index) pairs the handle's LAST sweep left in HBM (n = its k for gpx_sweep* / gpx_ensemble_sweep* / gpx_constrained_sweep* /
 * gpx_ehvi_* (the lead), S*k for gpx_rff/path_sweep*), taken straight from the device, `index_offset` (this rank's shard origin) added to every valid index.
 *   k > 0: every rank receives the same merged k best in out_val[k], out_idx[k] = the global argsort(finit)[::-1][:k] of pybo/solvers/lbfgs.py:51 over
 *          the sharded grid.
 *   k = 0: no merge; out_val / out_idx receive all nranks*n pairs in rank order (batch-BO: one recommendation per Thompson draw, draws sharded over ranks). */
int gpx_topk_allgather(gpx_comm *c, int64_t n, int64_t index_offset, int64_t k, double *out_val, int64_t *out_idx);
/* ---- measurement ------------------------------------------------------------------------ */
/* Stage timers in milliseconds accumulated since the last reset (HIP events on the handle's stream): [0] gram [1] cholesky [2] trtri [3] alpha [4] cross_gram
 * [5] sweep_trmm [6] acq_topk [7] rff [8] sweep_trmm launches [9] sweep_trmm algorithmic flop [10] h2d/d2h copies [11] append [12] correction passes over the
 * sweep cache [13] the Thompson sweep kernel alone (part of [7]) [14] its algorithmic fp64 lane operations, S n (d + 20) M per launch [15] fits whose
 * task-graph factorisation gave up and re-ran on the stream schedule [16] the shader clock in MHz the sweep_trmm launches sustained (their workgroups'
 * s_memtime over s_memrealtime ticks) [17] the same for the Thompson sweep kernel [18] inversions whose leading part ran behind the factorisation
 * ("trtri_ahead": for those [2] holds only what was left after the factor was done) [19] bound pass of selection-only sweeps [20] batch selection
 * (gpx_*sweep_batch*) [21] joint posterior (gpx_predict_cov / gpx_sample_joint: all between their copies).  Synchronises; returns slots written. */
int gpx_timers(gpx_handle *h, double *out, int n, int reset);
int gpx_diagnostics(void);     /* 1 when the library was built with -DGPX_DIAGNOSTICS (the diagnostic options above are accepted), else 0 */
int gpx_sync(gpx_handle *h);
#ifdef __cplusplus
}
#endif
#endif /* GPX_H */
