/*
 * gpx_diag.h -- diagnostic entry points and options of libgpx (NOT part of the shipping C-ABI, include/gpx.h).
 *
 * The entry points below are exported by every build (they only read).  The OPTIONS below (the DIAG rows of gpx_set_option's
 * table in api.hip) are accepted only by a library whose diag_flag.cpp was compiled with -DGPX_DIAGNOSTICS (build.sh builds
 * it next to the shipping one: pybo_amd/csrc/libgpx_diag.so; Python: GPX_DIAGNOSTICS=1 in the environment selects it,
 * tests/conftest.py does); the shipping libgpx.so answers them with GPX_EARG -- a consumer of include/gpx.h cannot switch
 * parts of a factorisation off by a typo.
 *
 *   "chol_tg_chunks"  k-chunk sizes of the task-graph factorisation counted back from the pivot as decimal digits (9 = 16 blocks)
 *                     [0 = by size: 112489 = 1, 1, 2, 4, 8, 16, 16, ..; up to 36 blocks 11112489]
 *   "chol_tg_nap"     longest pause of a waiting workgroup between two looks at its dependencies, x 64 clocks: 8, 16, 32, 64, 127 [16]
 *   "chol_tg_grid"    workgroups launched [0 = by size];  "chol_tg_isolate" 1: the critical workgroups keep their CUs to themselves [-1: up to 112 blocks]
 *   "chol_tg_trace"   1: stamp the critical path (gpx_chol_trace); 2: also a per-workgroup task log
 *   "grad_rb_cs"      columns per segment of the register-blocked triangular matvec, a multiple of 128 [0 = default]
 *   "x_rff"           1: the round-3 Thompson sweep kernel instead of the default (process-wide; A/B and witness of the tests)
 *   "x_bg", "x_bg_lds", "x_bg_iters"   a synthetic register-only fp64-MFMA kernel of x_bg workgroups (x_bg_lds KB of LDS each,
 *                     x_bg_iters rounds) runs beside the factorisation (scripts/chol_bg.py)
 *   "x_skip"          leave out the far updates (bit 0), the chain kernels (bit 1) or the near updates (bit 2) of the stream-scheduled
 *                     factorisation to time its parts alone -- the result is then NOT a factorisation
 *   "prune_keep"      1: a pruned selection-only sweep keeps a device copy of its bound vector and of its seed list as they are before
 *                     the seeds are scattered, and of the bound pass's dots (three device-to-device copies, no other change), for
 *                     gpx_prune_report and gpx_prune_dots [0]
 *   "prune_bound"     the kernel of a pruned sweep's bound pass: 0 the generic k_sweep_rankq<1>; 1 the matrix-pipe kernel wherever it exists
 *                     (SE-ARD, d <= 18), whatever its guard says; 2 the fp32 matrix-pipe kernel, which adds its own error margin to each
 *                     dot (csrc/bound_f32.h), wherever it exists, whatever the guards say; -1 by the guards, the fp32 kernel only from
 *                     131072 candidates on [-1]
 *   "bound_fact"      0: the fp32 kernel of the bound pass keeps the unfactorised exponent everywhere; 1: it walks the factorised form
 *                     (csrc/bound_f32.h: norm factors in the weights and once per candidate) wherever that form's guard allows [1]
 *   "prune_rows"      block rows of the row prefix behind a pruned sweep's second bound: 0 never (the
 *                     single bound alone); n > 0: min(n, nP, N / 128) rows wherever the first level pruned; -1 by size: nP / 4 rows where
 *                     M >= 32768, nP >= 32 and more than Gg candidates survived the first bound [-1]
 *   "short_map"       the short form of tile map 3 (csrc/sweep_map.h: an XCD owns a slice of the candidate tiles AND a slice of the pair rows):
 *                     0 never; 1 wherever map 3 is in use; -1 by size: launches whose ceil(NT / 8) tiles per XCD are fewer than a
 *                     super-tile's RES / super_m -- the results are the same bits under every value [-1]
 *   "prune_seeds"     the seed count G of a pruned sweep: 0 by the rule (prune_geom); n > 0: n rounded up
 *                     to a multiple of 32, and to at least k -- the top-k stays what it is, the lists and the launches change [0]
 */
#ifndef GPX_DIAG_H
#define GPX_DIAG_H
#include "../../include/gpx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ("chol_tg_trace" = 1) wall-clock stamps (100 MHz ticks) the task-graph factorisation of the last fit took with its own clock:
 * out[4 p + {0, 1, 2}] = the diagonal workgroup started waiting for / started / finished block p (nP = N/128 rounded up blocks),
 * then out[4 nP + 2 (8 p + i) + {0, 1}] = stamps of the shadows of block row p (i = 0: S1 started waiting for its right-hand sides /
 * has them loaded, 1: .. / its last rows are stored; 2, 3: the same for S2; 4: U started waiting / the tile's earlier chunks are in,
 * 5: the tile is loaded / stored for the diagonal workgroup).  Returns the number of words written (<= n; 20 nP when complete,
 * followed by up to 1024 x 8 per-workgroup counters: tasks, ticks spent taking / updating / solving / publishing, block updates
 * applied, role, exit stamp), 0 without a trace. */
int64_t gpx_chol_trace(gpx_handle *h, int64_t *out, int64_t n);

/* The task lists the task-graph factorisation of an nblocks x nblocks block matrix walks (host only, no device needed: what the CPU
 * tests replay to prove that every tile receives every block row once, in order, and that the lists never dead-lock):
 * counts[2] = entries of list 0 / tasks of the workers' list, out (total, 8) int16 = {type, I, J, k0, k1, ordinal, aux, reserved},
 * the lists back to back.  Types: 1 = panel solve of the 64-column half aux of tile (I, J); 2 = update of tile (I, J) with block rows
 * [k0, k1), its chunk number `ordinal`; 5 = a fused link: the solve of half aux of tile (I, J) and the final chunk [k0, k1 = I+1)
 * (chunk number `reserved`) of the same half of tile (I+1, J); 4 = list 0's descriptor of block row I for the workgroups that follow
 * the diagonal factorisation (they stand for the solves of tiles (I, I+1 .. I+3), the final chunks of tiles (I+1, I+1 .. I+3) =
 * [k0, k1) with chunk number aux, and the diagonal tile's chunk before it, which starts at block row `reserved` if that is >= 0;
 * `ordinal` = chunks of every tile of row I).  The lists are those of a launch with two k-step images of LDS per workgroup (fused
 * links).  chunks as the option "chol_tg_chunks" (<= 0: default).  Returns the total number of entries (written only when
 * cap >= total), -1 on bad arguments.  (Round 5's gpx_chol_tasks had a `split` argument and three counts: renamed, not re-used.) */
int64_t gpx_chol_tasks2(int nblocks, int chunks, int16_t *out, int64_t cap, int64_t *counts);

/* What the handle's LAST sweep decided about pruning and with what; it only copies what the sweep left behind.
 * scal[0 .. min(nscal, 22)) = { path: 0 plain (not legal or not tried), 1 the gate declined, 2 pruned, 3 the bound pass ran but more than
 * cap candidates survived and the plain loop evaluated everything;  M;  k;  G (seeds);  Gg (the gate's generation);  done (leading
 * candidates evaluated before the bound pass);  cap;  nsurv;  S;  delta;  tau (the k-th best seed value);  the gate's mean s2 (NaN: no
 * gate);  the seeds' threshold key;  1 if the kept copies exist;  the bound pass's kernel, 0 generic / 1 matrix pipe / 2 matrix pipe in fp32;  the guard's (d + 4) (R_x + R_z)^2
 * (NaN where the host chose the generic kernel: another covariance, d > 18, prune_bound = 0);  nR, the block rows of the second bound's
 * prefix (0: it did not run);  nsurv2, the survivors of its cut (the candidates evaluated exactly on path 2 where nR > 0);  E, the relative margin of the
 * fp32 kernel (csrc/bound_f32.h; NaN where that kernel was not considered);  1 if this sweep skipped its gate on the decision carried from the last one
 * (csrc/prune_hint.h; then done = 0 and the gate's mean is NaN), else 0;  1 if the fp32 kernel walked its factorised form, 0 if the unfactorised one;
 * tpos, the first 16-row tile of that kernel's reordered weights without a positive one (both NaN where it did not run) }.  S .. tau, the key, the guard and E are NaN for paths 0 and 1.
 * ub (optional, M): the bound vector as the survivor pass read it (-inf where a candidate was evaluated as gate or seed);  idx
 * (optional, cap_idx): the first min(nsurv, cap, cap_idx) survivors in the order they were compacted;  ub_kept (optional, M) and
 * seed_idx (optional, cap_seed; G entries): the bound vector and the seed list before the scatter -- only after a sweep that ran with
 * the option prune_keep = 1.  GPX_ESTATE: no sweep since the record was cleared, a vector was asked for and the last sweep's path is below 2, or a kept vector
 * was asked for and the sweep kept none.  (Every entry into gpx_sweep[_dev] and gpx_sweep_update[_dev] clears the record, a refused call
 * included -- the report then answers GPX_ESTATE; a sweep that passes its argument checks starts a new one; nothing else writes the workspace.) */
int gpx_prune_report(gpx_handle *h, double *scal, int nscal, double *ub, int64_t *idx, int64_t cap_idx, double *ub_kept,
                     int64_t *seed_idx, int64_t cap_seed);

/* dots (M): alpha2 . k(X, z_n) as the bound pass's kernel left them, before EI was taken of them -- only after a pruned sweep (path >= 2)
 * that ran with the option prune_keep = 1 (GPX_ESTATE otherwise). */
int gpx_prune_dots(gpx_handle *h, double *dots);

/* The second bound of the last sweep, only after a sweep with the option prune_keep = 1 that ran it (path 2 with nR > 0; GPX_ESTATE
 * otherwise), aligned with the first-level list `idx` of gpx_prune_report: ub2 (optional, nsurv) = EI((bias + dot) + delta,
 * max(rho - qR, S2_FLOOR));  qR (optional, nsurv) = the sum of V^2 over the leading nR block rows, added block by block as the exact
 * chain adds them;  idx2 (optional, cap_idx2): the first min(nsurv2, cap_idx2) candidates that survived the second cut, in order.
 * (An entry point of its own, so that gpx_prune_report keeps the signature its callers were built against.) */
int gpx_prune_rows(gpx_handle *h, double *qR, double *ub2, int64_t *idx2, int64_t cap_idx2);

/* What the LAST ensemble sweep led by members[0] decided about pruning; `members`, n as in that call.
 * scal[0 .. min(nscal, 11 + 2 n)) = { path 0 .. 3, M, k, G, Gg, done, cap, nsurv as in gpx_prune_report;  tau (NaN for paths 0 and 1);  the
 * gate's value, the mean over the members of mean(s2_m) / rho_m of its generation (NaN: no gate);  then delta_m of every member (NaN for
 * paths 0 and 1);  then, at 10 + n, 1 if this sweep skipped its gate on the lead's carried decision, else 0;  then per member 1 where its dots came from
 * the fp32 kernel's factorised walk, 0 from another kernel or form (NaN: the host chose the generic kernel, or paths 0 and 1) }.  ub (optional, M): the ensemble bound vector -- the members' bounds summed in member order and divided by n -- as the
 * survivor pass read it (-inf where a candidate was evaluated as gate or seed);  idx (optional, cap_idx): the first min(nsurv, cap,
 * cap_idx) survivors in the order they were compacted.  GPX_ESTATE: no ensemble sweep of n members since the record was cleared, or a vector
 * was asked for and the path is below 2.  (Every entry into gpx_ensemble_sweep[_dev] clears the lead's record, a refused call included;
 * so does a later sweep of the lead alone whose workspace has to grow.  The members' own gpx_prune_report records say path 0 afterwards.) */
int gpx_ensemble_prune_report(gpx_handle *const *members, int n_members, double *scal, int nscal, double *ub, int64_t *idx,
                              int64_t cap_idx);

/* What the LAST constrained sweep led by `lead` (the objective's handle, or cons[0] where there was none) decided about pruning (DESIGN.md
 * section 2.3).  scal[0 .. min(nscal, 11)) = { path 0 .. 3, M, k, G, Gg, done, cap, nsurv as in gpx_prune_report;  tau, the k-th best seed value
 * of the PRODUCT (NaN for paths 0 and 1);  the gate's value, the objective's mean s2 over its generation, not divided by rho (NaN: no gate);
 * delta of the objective's bound (NaN for paths 0 and 1) }.  ub (optional, M): the objective's EI bound as the survivor pass read it (-inf where
 * a candidate was evaluated as gate or seed);  idx (optional, cap_idx): the first min(nsurv, cap, cap_idx) survivors in the order they were
 * compacted.  GPX_ESTATE as gpx_ensemble_prune_report: every entry into gpx_constrained_sweep[_dev] clears the lead's record, a refused call
 * included; so does every later selection-only sweep of the lead, alone or as an ensemble's lead, that reaches its workspace (the three records'
 * vectors share it), and a constrained sweep that reaches it ends the lead's ensemble record likewise. */
int gpx_constrained_prune_report(gpx_handle *lead, double *scal, int nscal, double *ub, int64_t *idx, int64_t cap_idx);

#ifdef __cplusplus
}
#endif
#endif /* GPX_DIAG_H */
