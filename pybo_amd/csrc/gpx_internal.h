// gpx_internal.h -- handle layout and host-side launcher prototypes (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/gpx.h"
#include "acq_core.h"
#include "prune_hint.h"
#include "sweep_map.h"
#include "ws_layout.h"

namespace gpx {

constexpr int DMAX_RFF = DMAX;          // max input dimension of the Thompson / RFF kernels (round 3: the projection walks d in chunks)
constexpr int DMAX_RFF_RESIDENT = 64;   // up to here the whole k-range of a feature tile [d][144] lives in LDS at once
constexpr int TOPK_MAX = 4096;   // max k of the device top-k (served TOPK_PASS entries per pass)
constexpr int TOPK_PASS = 64;

enum Timer {
    T_GRAM = 0, T_CHOL, T_TRTRI, T_ALPHA, T_XGRAM, T_TRMM, T_ACQ, T_RFF, T_NLAUNCH, T_FLOP, T_COPY, T_APPEND,
    T_RANK1, T_RFFSWEEP, T_RFFOPS, T_TGFALL, T_SCLK, T_RFFCLK, T_AHEAD, T_BOUND, T_BATCH, T_JOINT, T_COUNT
};

struct EventPair { hipEvent_t a, b; int slot; };

}  // namespace gpx

struct CholGraphKey {             // what a captured factorisation depends on (compared bytewise: zero-filled before use)
    int64_t Np;
    int w, rl, merge, fuse;
    const void *S, *R, *T, *U, *flag;
    hipStream_t s2, s3, s4;
};

struct gpx_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;   // library-owned side stream (Cholesky lookahead: far trailing updates, low priority)
    hipStream_t stream3 = nullptr;   // library-owned side stream (rows 2..4 of the next panel's near update, normal priority)
    hipStream_t stream4 = nullptr;   // library-owned side stream (mid(P): the next-but-one panel's rows, low priority)
    hipEvent_t ev_chain = nullptr, ev_far = nullptr, ev_rest = nullptr;
    hipEvent_t ev_row[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int x_skip = 0;               // diagnostic: time parts of the factorisation alone (see launch_cholesky)
    int x_bg = 0, x_bg_lds = 72, x_bg_iters = 10000;   // diagnostic: synthetic MFMA background load (k_bg_mfma)
    hipStream_t stream_bg = nullptr;
    int chol_merge = 1;           // two-panel accumulation of the far updates while >= this many rest block rows (0 = off)
    int chol_fuse = 0;            // diagonal block + panel solve in one launch (k_potrf_solve16)
    int chol_graph = 0;           // replay the factorisation's launches from a captured hipGraph (per size / options / buffers)
    hipGraphExec_t chol_exec = nullptr;
    CholGraphKey chol_key;
    int chol_rl = 1;              // in-panel updates right-looking (1, default) or left-looking (0)
    int chol_w = 0;               // outer panel width of the factorisation in 128-blocks (2..8; 0 = by size)
    // the factorisation as ONE persistent task-graph kernel (kernels_chol_tg.hip)
    int chol_tg = 1;              // 1 (default): task-graph kernel for fits of >= tg_min blocks; 0: the stream schedule
    int tg_min = 2;               // smallest number of 128-blocks the task-graph kernel is used for (round 5, with the shadows: it wins from two blocks on, by the kernel's clock -- N = 256: 0.082 against 0.091 ms -- and, since the abort word travels with the pivot flag in ONE copy, by the host's: fit up to the factor 0.172 against 0.184 ms at N = 200, 0.213 against 0.236 at 300, 0.25 against 0.29 at 500, 0.41 against 0.54 at 1000)
    int tg_max = 160;             // ... and the largest (from N = 24576 on the stream schedule is 1-2 % faster: both throughput-bound)
    int tg_chunks = 0;            // chunk sizes counted back from the pivot, as decimal digits (0 = default by size: 112489 = 1, 1, 2, 4, 8, 16, 16, .., up to 36 blocks 11112489)
    int tg_nap = 0;               // longest polling pause of a waiting workgroup in units of 64 clocks (0 = default 16; round 4 until late: 127)
    int tg_db = -1;               // -1 (default): the double-buffered workers (one workgroup per CU, 2 x 72 KB of LDS) up to tg_db_max blocks; 0 / 1: never / always
    int tg_fuse = 1;            // a column's solve and the final chunk of the tile below it as one task (needs the shadows and one workgroup per CU)
    int tg_db_max = 112;          // (N = 12288: 13.04 against 13.38 ms; N = 16384: 27.6 against 27.2: two workgroups per CU win there)
    int tg_grid = 0;              // workgroups launched (0 = by size, bounded by residency)
    int tg_isolate = -1;          // the critical workgroups keep their compute units to themselves (full grids only): -1 by size (up to 112 blocks), 0 / 1
    int tg_trace = 0;             // diagnostic: stamp the critical path with the kernel's own clock (gpx_chol_trace)
    int tg_tmo_ms = 0;            // bound of every spin in milliseconds (0 = default 2000)
    bool tg_launched = false;     // the last factorisation ran on the task-graph kernel
    int tg_fallbacks = 0;         // launches that gave up (spin bound) and were re-run on the stream schedule
    void* tg = nullptr;           // its cached tables / control block (gpx::TgCache)
    std::string err;

    // model state
    bool fitted = false;
    int stage = 0;               // 0 none, 1 gram, 2 chol (fitted; T/U/a/alpha not formed yet), 3 + inverse
    int ahead_top = 0;               // != 0: the leading part of the inversion has been enqueued on stream2 behind the factorisation's gate (ev_rest marks its end)
    bool want_ahead = false;         // fit_core -> launch_cholesky_tg: the inverse follows at once (stage 3 / eager_inverse)
    int trtri_ahead = 1;             // option: allow that (task-graph factorisation with one workgroup per CU only)
    int trtri_ahead_min = 8;         // ... from this many blocks on (N = 1024: 0.43 -> 0.41 ms factor + inverse, 1536: 0.65 -> 0.58, 2560: 1.17 -> 1.05: below ~24 blocks the factorisation does not fill the chip and the side stream finds free compute units at once)
    bool diag_inv_pending = false;   // the diagonal blocks of T / U hold 16x16 inverses only (k_trtri_diag128 due)
    bool eager_inverse = false;  // option: form the inverse inside the fit (timing experiments)
    int grad_form = 0;           // option: predict-with-gradients form (0 auto: one pass for a single point, 1 two passes, 2 one pass)
    int grad_rb_cs = 0;          // option (experiment): columns per segment of k_tri_matvec_rb (0 = 2048)
    int grad_kernel = -1;        // option: triangular matvec of the two-pass form (-1 auto, 0 one wave per row, 1 register-blocked)
    int trtri_left = 0;          // option: the triangular inverse's recursion as -(T22 L21) T11 instead of -T22 (L21 T11) (measured: no better)
    bool refine_inverse = false; // option: one Newton step on the triangular inverse (left residual)
    double* drefine = nullptr;   // its Np^2 scratch (allocated on first use, capacity cap_np^2)
    int64_t cap_refine = 0;
    int64_t N = 0, Np = 0, d = 0;
    int kernel_id = 0;
    double rho = 1, sn2 = 0, bias = 0;
    std::vector<double> ell;
    int64_t fail_pivot = -1;

    // device buffers (capacity tracked in elements)
    int64_t cap_np = 0, cap_d = 0;
    double* dXs = nullptr;    // (Np, d) observed points scaled by 1/ell, padded rows = 0 (allocated (cap_np, cap_d))
    double* dXraw = nullptr;  // (N, d) observed points as given
    double* dy = nullptr;     // (Np,) y (padded 0)
    double* dS = nullptr;     // (Np,Np) working Gram matrix (upper), later trtri workspace
    double* dR = nullptr;     // (Np,Np) upper Cholesky factor, row-major: K = R^T R
    double* dT = nullptr;     // (Np,Np) T = R^-T (lower), row-major
    double* dU = nullptr;     // (Np,Np) U = R^-1 = T^T (upper), row-major
    double* da = nullptr;     // (Np,) a = T (y - bias)
    double* dalpha = nullptr; // (Np,) alpha = U a
    double* dinvell = nullptr;// (DMAX,) 1/ell
    double* hinv = nullptr;   // pinned host staging of 1/ell (DMAX doubles): its H2D copy needs no host synchronisation
    hipEvent_t ev_inv = nullptr;     // completion of that copy (waited for before the buffer is rewritten)
    bool inv_inflight = false;
    double* hpin = nullptr;   // pinned host staging of predict-with-gradients (GB points)
    int64_t cap_hpin = 0;
    double* hpin_dev = nullptr;   // the same buffer as the device sees it (single-point results are written there directly)
    char* dsmall = nullptr;   // ONE allocation behind dflag / dscal / dinvell / dclk
    unsigned long long* dclk = nullptr;   // {sum of s_memtime ticks, sum of 100 MHz ticks} over the sweep kernel's workgroups: the sustained shader clock
    int* dflag = nullptr;     // [0] = failing pivot + 1 (0 = ok)
    double* dscal = nullptr;  // small scalar scratch (16 doubles)

    // sweep workspace
    int64_t chunk = 0;        // option: candidate columns per chunk (multiple of 128); 0 = by size: 65536, 131072 up to N = 4096 (half the launches: config B 68.4 -> 68.0 ms)
    int super_m = 8;          // rows (mt) of an XCD super-tile of 64 workgroups: 8 -> 8x8, 4 -> 4x16, 2 -> 2x32
    int tile_order = -1;      // -1: by size (7 below 32 block rows, 19 from there on); else bits 0-1 tile map (3 = XCD 8x8 super-tiles of PAIRED tiles), bits 2-4 k-loop schedule (launch_sweep_trmm)
    int64_t cap_ks = 0;       // elements of dKs
    double* dKs = nullptr;    // cross-Gram chunk, tile-blocked [chunk/128][Np][128]
    double* dQp = nullptr;    // (Np/128, chunk) per-row-block partials of colsum(V^2)
    double* dPp = nullptr;    // (Np/128, chunk) per-row-block partials of V^T a
    int64_t cap_part = 0;
    double* dXc = nullptr;    // staging for host candidates (M, d)
    int64_t cap_xc = 0;
    double* dout = nullptr;   // staging for host outputs 3*(M) (acq, mu, s2)
    int64_t cap_out = 0;
    double* dblkv = nullptr;  // per-block top-k values
    int64_t* dblki = nullptr; // per-block top-k indices
    int64_t cap_blk = 0;
    int64_t cap_blki = 0;
    double* dtopv = nullptr;  // final top-k (S*k)
    int64_t* dtopi = nullptr;
    int64_t cap_top = 0;
    const double* last_topv = nullptr;   // device (value, index) pairs of the last sweep's top-k, read by
    const int64_t* last_topi = nullptr;  // gpx_topk_allgather
    int64_t last_topn = 0;
    double* drff = nullptr;   // RFF parameter staging
    int64_t cap_rff = 0;
    double* drffs = nullptr;  // RFF feature-Gram scratch (Phi slabs + split-K partials)
    int64_t cap_rffs = 0;
    double* dgrad = nullptr;  // scratch of predict-with-gradients, gpx_append and gpx_rff_grad (grad_ws, append_ws, rff_grad_ws)
    int64_t cap_grad = 0;
    double* dens = nullptr;   // ensemble sweep: accumulators + member outputs (ens_ws)
    int64_t cap_ens = 0;
    double* dcon = nullptr;   // constrained sweep: one constraint's probabilities + the running product (con_ws)
    int64_t cap_con = 0;
    double* dehvi = nullptr;  // two-objective sweep: the members' four moment vectors, the values, the front's strips (ehvi_ws)
    int64_t cap_ehvi = 0;
    double* dehvib = nullptr; // two-objective batch picks: the lead's strips at capacity, believed outcomes, front sizes (ehvi_batch_ws)
    int64_t cap_ehvib = 0;
    int prune = -1;          // option: selection-only sweeps skip candidates whose EI bound cannot reach the top-k (-1 by size and gate, 0 never, 1 wherever legal)
    char* dprune = nullptr;   // their workspace (one allocation: prune_ws_layout)
    int64_t cap_prune = 0;    // ... in bytes
    // What the last selection-only sweep decided: the head both records share, filled by select_topk_pruned (api.hip) -- host scalars and
    // where the sweep's vectors lie in the lead's dprune
    struct SelectRecord {
        int path = -1;            // -1 no sweep yet, 0 plain, 1 the gate declined, 2 pruned, 3 bound pass ran but too many survived
        int64_t M = 0, k = 0, G = 0, Gg = 0, done = 0, cap = 0, nsurv = 0;
        double gate = 0.0;        // the gate's value (NaN where it did not run): the single model's mean s2, NOT divided by rho; the ensemble's
                                  // mean over the members of mean(s2_m) / rho_m
        bool hinted = false;      // the gate was skipped on the carried decision (prune_hint.h)
        const double* ub = nullptr;
        const int64_t* idx = nullptr;
        const double* sc = nullptr;       // sc[5] = tau as the survivor pass cut with it
    };
    // the last sweep of this handle (gpx_prune_report, gpx_diag.h)
    struct PruneRecord : SelectRecord {
        const int* st = nullptr;
        int bound_kernel = -1;    // -1: sc[9] says which kernel wrote the dots; 0: the host chose k_sweep_rankq<1> (no guard ran)
        bool kept = false;        // dkeep holds this sweep's bound vector and seed list as they were before the scatter
        // the second level (row-prefix bound): nR = 0 where it did not run; its vectors lie in dprune like the first level's
        int nR = 0;
        int64_t nsurv2 = 0;
        const double *qR = nullptr, *ub2 = nullptr;      // aligned with idx (qR only under prune_keep)
        const int64_t* idx2 = nullptr;
    } prune_rec;
    // the last ENSEMBLE sweep led by this handle (gpx_ensemble_prune_report): its vectors lie in this handle's dprune
    struct EnsPruneRecord : SelectRecord {
        int n = 0;
        const double* delta = nullptr;    // n: the members' delta_m
    } ens_rec;
    // the last CONSTRAINED sweep led by this handle (gpx_constrained_prune_report): its vectors lie in this handle's dprune
    struct ConPruneRecord : SelectRecord {
        int nc = 0;
    } con_rec;
    // the gate's decision carried to the next sweep of the same shape (prune_hint.h): this handle's own sweeps / the ensemble sweeps it
    // leads.  NOT part of the records: those are reset by every sweep entry and by a growing workspace.  Dropped by any gpx_set_option.
    gpx::PruneHint prune_hint, ens_hint;
    int prune_keep = 0;       // diagnostic option: keep those two device copies
    int prune_bound = -1;     // diagnostic option: the bound pass's kernel (-1 by guard, 0 k_sweep_rankq<1>, 1 k_bound_mfma / 2 k_bound_mfma32 wherever SE-ARD, d <= 18)
#ifdef GPX_BOUND32_NOFACT
    int bound_fact = 0;       // (A/B build: sign tiles alone)
#else
    int bound_fact = 1;       // diagnostic option: 0 the fp32 bound kernel keeps the unfactorised exponent, 1 the factorised form where its guard allows (bound_f32.h)
#endif
    int prune_rows = -1;      // diagnostic option: block rows of the second bound's row prefix (-1 by size: nP / 4, 0 never, n > 0: min(n, nP, N / 128) wherever the first level pruned)
    int sweep_cols = -1;      // option: candidate columns of a sweep workgroup's tile (sweep_shape_of): -1 by size, 128 / 64 / 32 forced
    int sweep_images = -1;    // option: LDS images of the default sweep schedule's k-loop (sweep_shape_of): -1 by size, 1 / 2 forced
    int prune_seeds = 0;      // diagnostic option: the seed count G of a pruned sweep (0: by the rule, api.hip: prune_geom)
    int short_map = -1;       // diagnostic option: the short form of tile map 3 (sweep_map.h) -1 by size (launches that cannot fill the per-XCD patches), 0 never, 1 always
    char* dkeep = nullptr;    // the diagnostic copies (keep_ws)
    int64_t cap_keep = 0;     // ... in bytes

    // sweep cache (warm BO step): candidates and their reduced sums q = colsum(V^2), p = V^T a of the last full
    // sweep, kept current by gpx_append's rank-1 correction and re-scored by gpx_sweep_update
    const double* app_w = nullptr;   // scratch of the last gpx_append: w = K^-1 k(X, x_new)
    bool cache_on = false;       // option "sweep_cache"
    bool cache_valid = false;
    int64_t cache_M = 0;
    double* dcZ = nullptr;       // (M, d) candidates
    double* dcq = nullptr;       // (M,) q, then p (one allocation: dcp = dcq + cap_cq / 2)
    double* dcp = nullptr;
    int64_t cap_cz = 0, cap_cq = 0;
    // appended observations whose cache correction is still due (applied together, at most PEND_MAX per pass)
    double* dpend = nullptr;     // the queued weight rows of pitch pend_ld and their scalars (pend_ws)
    int64_t pend_ld = 0;
    int npend = 0;

    // announced observation (gpx_append_begin): the y-independent part of the next append and the correction pass of
    // the sweep cache run ahead, on the third stream, while the caller evaluates its objective
    bool spec_active = false;    // an announcement is waiting for its gpx_append
    bool spec_launched = false;  // the third stream may still be reading the announcement's buffers
    bool spec_used = false;      // the last append_host consumed the announcement (api.hip finishes the cache update)
    bool apply_pending = false;  // ... whose q += v^2, p += v a is still due (applied by flush_pending)
    uint64_t gen = 0, spec_gen = 0;      // model generation (fit / append / grow) now and at the announcement
    std::vector<double> spec_x;  // the announced point (host copy, compared bit for bit)
    double* dspec = nullptr;     // the announcement's buffers (spec_ws)
    int64_t cap_spec = 0, spec_ld = 0, spec_M = 0;
    hipEvent_t ev_spec_go = nullptr, ev_spec_done = nullptr;

    // batch proposals (gpx_sweep_batch): scratch of its own (batch_ws) -- nothing the append / announcement paths own
    double* dbsel = nullptr;
    int64_t cap_bsel = 0;
    std::vector<gpx::BatchMember> bsel_desc;      // host source of the lead's descriptor table (gpx_ensemble_sweep_batch): outlives its copy
    double* dfant = nullptr;                      // gpx_sweep_batch_fantasy: innovations, incumbents, forced rows (fant_ws)
    int64_t cap_fant = 0;
    std::vector<unsigned char> fant_host;         // host source of that upload: outlives its copy

    // joint posterior (gpx_predict_cov / gpx_sample_joint): scratch of its own (joint_ws); the cross-Gram of the points goes
    // through dKs like a sweep's
    double* djoint = nullptr;
    int64_t cap_joint = 0;

    // knowledge gradient (GPX_ACQ_KG, gpx_kg_grad; kernels_kg.hip): the prepared support set (kg_ws), kept while the model (gen) and
    // the set (kg_A) stay what they were, and work space of a sweep (C: 128 x chunk) or of gpx_kg_grad's point panels (kg_point_ws)
    double* dkg = nullptr;
    int64_t cap_kg = 0;
    double* dkgw = nullptr;
    int64_t cap_kgw = 0;
    std::vector<double> kg_A;    // the support set dkg was prepared for (empty: none)
    uint64_t kg_gen = 0;
    int64_t kg_Np = 0;

    // pathwise Thompson draws (gpx_path_weights / gpx_path_sweep / gpx_path_grad; kernels_path.hip): scratch of its own
    // (path_weights_ws, path_sweep_ws, path_grad_ws)
    double* dpath = nullptr;
    int64_t cap_path = 0;

    double* dbatch = nullptr;    // gpx_loglik_batch: one allocation (loglik_batch_ws)
    int64_t cap_batch = 0;
    double* dhyper = nullptr;    // gpx_loglik_grad: the tiles' partial sums and the result (hyper_ws; on first use)
    int64_t cap_hyper = 0;

    // timers
    std::vector<gpx::EventPair> pending;
    std::vector<hipEvent_t> pool;
    double tacc[gpx::T_COUNT] = {0};
};

namespace gpx {

// The grow-only allocation behind every workspace (api.hip): on GPX_OK p holds at least `need` elements; a buffer that has to grow is freed
// first (hipFree waits for the whole device).  `what`: "<what>: device allocation failed" with GPX_EOOM; without it the HIP call and its error.
int ensure_bytes(gpx_handle* h, void** p, int64_t* cap, int64_t need, size_t elem, const char* what);
template <typename T> inline int ensure(gpx_handle* h, T*& p, int64_t& cap, int64_t need, const char* what = nullptr) {
    return ensure_bytes(h, reinterpret_cast<void**>(&p), &cap, need, sizeof(T), what);
}

// launchers (kernels_fit.hip)
void launch_scale_x(hipStream_t s, const double* X, int64_t n, int64_t np, int d, const double* invell,
                    double* Xs);
void launch_gram_sym(hipStream_t s, const double* Xs, int64_t N, int64_t Np, int d, int kernel_id,
                     double rho, double sn2, double* S);
int ensure_side_streams(gpx_handle* h);   // api.hip: streams 2 / 3 + events, on first use
void launch_cholesky(gpx_handle* h);   // S -> R, diag blocks of T/U; sets dflag
bool launch_cholesky_tg(gpx_handle* h);    // the same by the persistent task-graph kernel (kernels_chol_tg.hip); false: not launched
int tg_abort_code(gpx_handle* h);          // after the stream has drained: 0 ok, 1 not PD, 2 a spin gave up
int64_t tg_trace_copy(gpx_handle* h, long long* out, int64_t n);
void tg_free(gpx_handle* h);
int64_t tg_tasks_copy(int nP, int chunks, int16_t* out, int64_t cap, int64_t* counts);
void launch_trtri(gpx_handle* h);      // R, diag blocks -> T, U (uses S as workspace)
void launch_trtri_ahead(gpx_handle* h, hipStream_t s, int top);   // the part that needs the leading `top` block rows only
int trtri_top(int nP);
void launch_refine_inverse(gpx_handle* h, double* tmp);   // option refine_inverse: one Newton step on T / U (tmp: Np^2 scratch)
void launch_alpha(gpx_handle* h);      // a = T (y - bias); alpha = U a
void launch_kinv_diag(gpx_handle* h, double* out);   // out[i] = [K^-1]_ii = sum_m U[i][m]^2
void launch_transpose_lower(hipStream_t s, const double* R, int64_t Np, double* out, int64_t N);
void launch_cholesky_small(hipStream_t s, double* S, double* R, int64_t np, int* flag);   // S (upper 128-block triangle, identity padding; consumed) = R^T R
void launch_posterior_wide(hipStream_t s, const double* A, const double* v, const double* z, int n, int64_t np, double sc,
                           double sn2, double* B, double* R, double* work, int* flag, double* theta);   // n >= 128 features

// launchers (kernels_sweep.hip)
// rows: the observed rows [0, rows) filled in every panel of pitch ldk (Np, or the leading nR 128 <= N of a row-prefix pass)
void launch_cross_gram(hipStream_t s, const double* Xs, int64_t rows, int64_t N, int d, const double* Xc,
                       int64_t m0, int64_t M, int64_t cols, const double* invell, int kernel_id,
                       double rho, double* Ks, int64_t ldk);
// nR: the block rows [0, nR) the launch covers (Np / 128: the sweep; fewer: a row-prefix launch, whose Qp / Pp[mt < nR] are the full launch's bits)
void launch_sweep_trmm(hipStream_t s, const double* U, int64_t Np, int nR, const double* Ks, int64_t ldk,
                       int64_t cols, const double* a, double* Qp, double* Pp, int64_t ldp,
                       int tile_order, int super_m, unsigned long long* clk, int short_map = -1, int64_t valid = -1, int sweep_cols = 128,
                       int sweep_images = 1);
// The shape of that launch's tiles (sweep_map.h: sweep_shape_of; SWEEP_NARROW_MIN_NP lives there too): 128, or 64 / 32 candidate
// columns (narrow tiles: kernels_sweep.hip, sweep_tiles) on one LDS image or two -- the same bits in every shape.  sweep_cols,
// sweep_images: the options (-1: by size; else that value wherever instances exist, i.e. on the default k-loop).  valid <= cols: the
// columns that hold candidates; the columns of narrow tiles past them are not computed.
// reduce partials, form mu/s2/acq for columns [0,cols) of this chunk -> global candidate m0+..
// nrb = 0: Qp/Pp are reduced per-candidate sums (the sweep cache); qsum/psum (optional) receive the reduced sums
void launch_acq(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0,
                int64_t cols_valid, double rho, double bias, int acq_id, double p0, double* acq_out,
                double* mu_out, double* s2_out, double* qsum, double* psum);
// the same for GPX_ACQ_MES (kernels_mes.hip): the sampled maxima by value (MesArg: mes_math.h)
struct MesArg;
void launch_acq_mes(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0,
                    int64_t cols_valid, double rho, double bias, const MesArg& ys, double* acq_out,
                    double* mu_out, double* s2_out, double* qsum, double* psum);
// launchers (kernels_kg.hip): W = U V for one k-major panel V [Np][128] (rows >= N, columns >= m: zeros); C[j][c] = sum_n B[n][j] Ks[c's panel][n][c]
// for the chunk's cols columns; k_acq's moments + the knowledge gradient of candidate m0 + n over the lines of the prepared support
void launch_kg_solve(hipStream_t s, const double* U, int64_t Np, int64_t N, int m, const double* V, double* W);
void launch_kg_cross(hipStream_t s, const double* B, int64_t Np, const double* Ks, int64_t ldk, int64_t cols, double* C, int64_t ldc);
void launch_acq_kg(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0, int64_t cols_valid,
                   double rho, double bias, double sn2, int kid, int d, const double* X, const double* invell, const double* As, int m,
                   const double* al, const double* C, int64_t ldc, double* acq_out, double* mu_out, double* s2_out, double* qsum,
                   double* psum);
// gpx_kg_grad: the sums of np <= 128 points (S: np (d + 1) 132) and value + gradient from them (L: 4 x 129 x 128 scratch)
void launch_kg_point_sums(hipStream_t s, const double* Xs, int64_t N, int d, const double* Z, int np, const double* invell, int kid,
                          double rho, const double* B, const double* alpha, const double* Wz, const double* Vz, double* S);
void launch_kg_point_final(hipStream_t s, const double* S, int np, int d, const double* Z, const double* invell, const double* As,
                           int m, const double* al, int kid, double rho, double bias, double sn2, double* L, double* f, double* g);
// correction of the cached sums after q <= 8 appended observations in one pass (see kernels_sweep.hip)
void launch_pend_store(hipStream_t s, const double* w, int64_t Nj, int64_t ldw, const double* scal, double* row,
                       double* pscal_j);
void launch_cache_apply(hipStream_t s, const double* v, const double* scal, int64_t M, double* qsum, double* psum);
void launch_scale_point(hipStream_t s, const double* x, const double* invell, int d, double* xs);
void launch_sweep_rank1_v(hipStream_t s, const double* Xs, int64_t Ntot, int d, const double* Wq, int64_t ldw,
                          const double* pscal, const double* Z, int64_t M, const double* invell, int kernel_id,
                          double rho, const double* xlast, double* vout, const double* skip = nullptr);
void launch_sweep_rankq(hipStream_t s, const double* Xs, int64_t Ntot, int d, const double* Wq, int64_t ldw, int q,
                        const double* pscal, const double* Z, int64_t M, const double* invell, int kernel_id,
                        double rho, double* qsum, double* psum);
// block-local top-k over vals[0..M) then merge -> topv/topi (k entries)
void launch_topk(hipStream_t s, const double* vals, int64_t M, int k, double* blkv, int64_t* blki,
                 int64_t nblk, double* topv, int64_t* topi);
// merge n candidate (value, index) pairs (index == INT64_MAX: no entry; consumed in place) into the k best
void launch_topk_merge(hipStream_t s, double* vals, int64_t* idx, int64_t n, int k, double* topv, int64_t* topi);
void launch_topk_rows(hipStream_t s, const double* vals, int64_t M, int64_t S, int k, double* blkv, int64_t* blki,
                      int64_t nblk, double* topv, int64_t* topi);
// selection-only sweeps: weights and error bound of the bound pass, the bound itself, radix select of the G-th largest
// bound, stable compaction (mode 0: seeds by the selected threshold st[2]; mode 1: survivors of the cut *tau), scatter
void launch_prune_alpha(hipStream_t s, const double* U, int64_t Np, const double* a, double rho, double bias, double* alpha2,
                        double* sabs, double* sc);
// the bound pass's dot for SE-ARD with the distances on the matrix pipe: KS = k-steps of its inner product (0: not for this model),
// workspace words, and prologue + guard + kernel (sc[9] = 1.0: one of them wrote `out`; 0.0: launch_sweep_rank1_v(.., skip = sc + 9) does)
constexpr int BM_SC_RX2 = 6, BM_SC_RZ2 = 7, BM_SC_GUARD = 8, BM_SC_USE = 9;      // slots of sc[] (0 .. 5: k_prune_delta, gate, tau)
// the fp32 link (bound_f32.h): E, 1.0 where a weight is outside fp32's normal range, 1.0 where k_bound_mfma32 writes the dots
// (sc[USE] is 1.0 then as well: the generic kernel skips on it, k_bound_mfma on this one), the margin's factor and flush term
// (sc[BADW]: 1.0 a weight w outside the range, 0.5 only a scaled weight w' of the factorised form).
// TPOS32: the fp32 copies' tiles [0, tpos) hold only w >= 0, the rest only w <= 0 (k_bound_aug); FACT32: 1.0 where the factorised walk runs
constexpr int BM_SC_E32 = 10, BM_SC_BADW = 11, BM_SC_USE32 = 12, BM_SC_FAC32 = 13, BM_SC_FLUSH32 = 14, BM_SC_TPOS32 = 15, BM_SC_FACT32 = 16;
int bound_mfma_ks(int kernel_id, int d);
void launch_bound_mfma(hipStream_t s, const double* Xs, int64_t N, int64_t Np, int d, const double* alpha2, double rho,
                       const double* Z, int64_t M, const double* invell, int force, bool allow32, bool allow_fact, double* ws, double* sc,
                       double* out);
// the fp32 link's kernels alone (kernels_bound32.hip; launch_bound_mfma calls it behind its guard): operands as k_bound_aug wrote them,
// Np + 16 rows in ntile tiles; WF32: the scaled weights of the factorised walk, which runs instead where sc[FACT32] says so
void launch_bound_mfma32(hipStream_t s, const float* A32, const float* W32, const float* WF32, const float* NX32, int KS, bool nc, int ntile, int d,
                         const double* Z, int64_t M, const double* invell, const double* cen, const double* sc, double* out);
void launch_prune_ub(hipStream_t s, const double* dots, double* ub, int64_t M, int64_t skip, const double* sc, double rho,
                     double bias, double p0);
// the second bound: ub2[j0 + n] = EI((bias + dots[idx[j0 + n]]) + delta, fmax(rho - sum_{rb < nR} Qp[rb][n], S2_FLOOR)) for the chunk's
// cols_valid survivors (qR_out, optional: the sums); idx2[j] <- idx[idx2[j]] after the second cut's compaction of list positions
void launch_prune_ub2(hipStream_t s, const double* Qp, int64_t ldp, int nR, int64_t j0, int64_t cols_valid, const int64_t* idx,
                      const double* dots, const double* sc, double rho, double bias, double p0, double* ub2, double* qR_out);
void launch_sel_remap(hipStream_t s, const int64_t* idx, int64_t* idx2, int64_t n);
// the ensemble's bound: one member's EI bound folded into the running sum (k_ens_accum's addition), then the sum / n (k_ens_finish's)
void launch_prune_ub_fold(hipStream_t s, const double* dots, double* acc, int64_t M, const double* sc, double rho, double bias,
                          double p0, int first, double* delta_out, int guarded, double* fact_out);
void launch_prune_ub_mean(hipStream_t s, double* acc, int64_t M, int64_t skip, double n);
void launch_prune_mean(hipStream_t s, const double* v, int64_t n, double* out);
void launch_sel_threshold(hipStream_t s, const double* v, int64_t M, int G, int* hist, int* st);
void launch_sel_compact(hipStream_t s, const double* v, int64_t M, int mode, const int* st, const double* tau, int64_t* blk,
                        int64_t cap, const double* Xc, int d, int64_t* idx, double* Xg, double* tau_seen = nullptr);
void launch_sel_scatter(hipStream_t s, const int64_t* idx, const double* vals, int64_t n, double* out, double* mark);
void launch_fill_neg_inf(hipStream_t s, double* out, int64_t from, int64_t M);

// predict with gradients (small M path)
int ensemble_predict_grad_host(gpx_handle* const* mem, int n, const double* Xc, int64_t M, double* mu, double* s2,
                               double* dmu, double* ds2);
int predict_mean_host(gpx_handle* h, const double* Xc, int64_t M, double* mu, double* dmu);
int predict_grad_host(gpx_handle* h, const double* Xc, int64_t M, double* mu, double* s2, double* dmu,
                      double* ds2);

// form T, U, a, alpha if the current fit has not done so yet (api.hip)
int ensure_inverse(gpx_handle* h);

int loglik_host(gpx_handle* h, double* out);
void launch_loglik(gpx_handle* h, double* out);   // kernels_grad.hip: the evidence of the current fit (a, R formed) -> out[0] on the device
int loglik_grad_host(gpx_handle* h, double* loglik, double* grad);   // kernels_hyper.hip
int loglik_batch_host(gpx_handle* h, int64_t B, const double* hyp, double* out);   // kernels_fit.hip
int append_host(gpx_handle* h, const double* x, double ynew);
// the y-independent kernels of an append, enqueued on s: k* = k(X, x), r = T k*, {d, 1/d, (resid - r.a)/d, d^2} -> scal
// (a non-positive d^2 sets *flag), tu = U r.  dx: the point on the device.
int grow_factor_if_full(gpx_handle* h);
void launch_append_prepare(gpx_handle* h, hipStream_t s, const double* dx, double* dks, double* dg, double* dr,
                           double* dtu, double resid, double* scal, int* flag);
// the announcement's buffers as gpx_append_begin sized them (spec_ld, spec_M)
inline SpecBuf spec_layout(const gpx_handle* h) { return spec_ws(WsCarver(h->dspec), (h->cap_d + 63) / 64 * 64, h->spec_ld, h->spec_M); }
int rff_grad_host(gpx_handle* h, const double* W, const double* b, const double* theta, int64_t n, int64_t d,
                  double bias, const double* Xc, int64_t M, double* f, double* g);

// launchers (kernels_batch.hip): one scoring pass (j < 0: round 0; else fold row j of V first) with per-block argmax partials
// (batch_blocks(M) of them), and the one-workgroup pick that merges them and leaves everything round j + 1 needs on the device.
// e: the model's batch state; b: the scratch that holds what a batch shares (taken, partials, picks, x); f: the fantasised form
// (EI / PI; update: move the incumbents after pick j, which reads row j of eps), NULL: the believer's
int batch_blocks(int64_t M);
void launch_batch_score(hipStream_t s, int j, int64_t M, const BatchMember& e, const BatchBuf& b, int acq_id, double p0, const FantArg* f,
                        double* s2_out);
void launch_batch_pick(hipStream_t s, int j, int64_t M, int d, const double* Z, const BatchMember& e, const BatchBuf& b, const FantArg* f,
                       bool update);
// the ensemble forms: ONE scoring pass with all n members of the device table `mem` inside it (each member's fold, its value or moments
// summed in member order, one division), the pick that leaves every member's next round on the device (b.ens_s2: (n, nb) member-major),
// and the bitwise compare of two candidate sets (*flag <- 1 where a 64-bit word differs)
void launch_ens_batch_score(hipStream_t s, int j, int n, int64_t M, const BatchMember* mem, const BatchBuf& b, int acq_id, double p0);
void launch_ens_batch_pick(hipStream_t s, int j, int n, int64_t nb, int64_t M, int d, const double* Z, const BatchMember* mem,
                           const BatchBuf& b);
void launch_ens_same_grid(hipStream_t s, const double* Za, const double* Zb, int64_t words, int* flag);
// the constrained form's scoring pass over the same table (the objective first where a.has_obj): con_chain of the members' terms; its pick is
// launch_ens_batch_pick
void launch_con_batch_score(hipStream_t s, int j, int n, int64_t M, const BatchMember* mem, const BatchBuf& b, const ConBatchArg& a);
// the two-objective form over a table of the two members: EHVI over the strips w.a / w.b of the w.n[0] points the device holds, and the
// pick that records the believed outcome (the members' means at the pick) and, unless it was the last, takes it into the strips
void launch_ehvi_batch_score(hipStream_t s, int j, int64_t M, const BatchMember* mem, const BatchBuf& b, const EhviBatchWs& w);
void launch_ehvi_batch_pick(hipStream_t s, int j, int64_t nb, int64_t M, int d, const double* Z, const BatchMember* mem, const BatchBuf& b,
                            const EhviBatchWs& w, bool last);

// launchers (kernels_cov.hip): the joint posterior at cols = Mp padded points -- V = T Ks stored panel-major [cols / 128][Np][128],
// mu = bias + V^T a (Pp: Np / 128 x cols partial sums), C = Kss - V^T V (Mp, Mp) symmetric bit for bit, B = C + add I with identity
// padding, out[s][j] = mu[j] + sum_{i <= j} z[s][i] R[i][j] (skipped when *flag != 0)
void launch_cov_trmm(hipStream_t s, const double* U, int64_t Np, const double* Ks, int64_t cols, double* V);
void launch_cov_mu(hipStream_t s, const double* V, int64_t Np, int64_t cols, const double* a, double bias, double* Pp, double* mu);
void launch_cov_syrk(hipStream_t s, const double* V, int64_t Np, const double* Kss, int64_t Mp, double* C);
void launch_cov_form(hipStream_t s, const double* C, int64_t M, int64_t Mp, double add, double* B);
void launch_cov_draw(hipStream_t s, const double* R, int64_t Mp, int64_t M, const double* z, int64_t S, const double* mu,
                     const int* flag, double* out);

// launchers (kernels_rff.hip)
extern int g_rff_variant;
void launch_rff_mfma(hipStream_t s, const double* Wt, const double* bt, const double* tt, int S, int nfb, int n, int d,
                     int dp, double bias, const double* Xc, int64_t M, double* vals, unsigned long long* clk);
int64_t rff_gram_batch_scratch(int64_t S, int64_t Np);
void launch_rff_posterior(hipStream_t s, const double* A, const double* v, const double* z, int S, int n, double sc,
                          double sn2, double* theta, int* flag);
void launch_rff_gram_batch(hipStream_t s, const double* Xraw, int64_t N, int64_t Np, int d, int dp,
                           const double* Wt, const double* bt, int S, int n, const double* y, double bias,
                           double* scratch, double* A, double* v);
void launch_rff_gram(hipStream_t s, const double* Xraw, const double* Ft_scratch, int64_t N, int d,
                     const double* W, const double* b, int n, const double* y, double bias, double* A,
                     double* v);

// launchers (kernels_path.hip): the update term of S pathwise draws added to vals (S, M), which holds the feature part (v: the device
// copy of the weights (S, nv), frag: path_frag_words(S, nv) doubles); the right-hand sides of the weights as panels of 128 draws, and
// the panels of U T r back to (S, N)
void launch_path_update(hipStream_t s, const double* Xs, int d, const double* v, int64_t nv, int64_t S, double* frag,
                        const double* Xc, int64_t M, const double* invell, int kernel_id, double rho, double* vals);
void launch_path_resid(hipStream_t s, const double* y, double bias, const double* prior, const double* eps, double sn, int64_t S,
                       int64_t N, int64_t Np, int64_t Sp, double* R);
void launch_path_gather(hipStream_t s, const double* Wp, int64_t S, int64_t N, int64_t Np, double* v);
// (kernels_grad.hip) value and gradient of one pathwise draw at M points
int path_grad_host(gpx_handle* h, const double* W, const double* b, const double* theta, const double* v, int64_t nv, int64_t n,
                   int64_t d, double bias, const double* Xc, int64_t M, double* f, double* g);

// launchers (kernels_ens.hip)
void launch_ens_accum(hipStream_t s, double* acc0, double* acc1, const double* t0, const double* t1, int64_t M,
                      int mode, int first);
void launch_ens_finish(hipStream_t s, const double* acc0, const double* acc1, int64_t M, int mode, double n,
                       double beta, double* out, double* mu_out, double* s2_out);
void launch_con_fold(hipStream_t s, double* v, double* w, const double* p, int64_t M, int first);
// (kernels_ehvi.hip) mom (4, M): mu1, s2_1, mu2, s2_2; strips: a then b, n + 2 doubles each, n <= EHVI_MAX_FRONT
void launch_ehvi_fold(hipStream_t s, const double* mom, int64_t M, const double* strips, int n, double* out);
void launch_grid_sobol(hipStream_t s, const uint32_t* sv, int bits, int64_t first, int64_t M, int d,
                       const double* bounds, double* X);
void launch_grid_uniform(hipStream_t s, uint64_t seed, int64_t first, int64_t M, int d, const double* bounds,
                         double* X);

}  // namespace gpx
