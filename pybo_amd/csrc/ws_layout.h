// ws_layout.h -- every device workspace of the library, described once.  Plain C++17 for the host: no HIP type, no handle.
//
// Each workspace is one grow-only allocation carved into typed regions.  Its walk below -- a function of plain sizes and a carver --
// is the ONLY description of the layout: called on a null base it sizes the allocation (the struct's `bytes`), called on the real base
// it hands out the pointers.  The order of the take() calls is the order in memory.  tests/c/ws_layout_check.cpp runs every walk over
// the shapes at which the arithmetic can go wrong and records the regions (tests/golden/ws_layouts.json).
#pragma once
#include <assert.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "bound_f32.h"
#include "kg_math.h"

namespace gpx {

constexpr int NB = 128;       // factorisation block = GEMM tile edge
constexpr int TBH = 128;      // host-side copy of the GEMM tile edge (gemm_core.h TB)
constexpr int DMAX = 1024;    // max input dimension (buffer sizing only: the kernels walk coordinates 16 at a time)
constexpr int PEND_MAX = 8;   // appended observations per pass of the sweep-cache correction
constexpr int GB = 16;        // candidates per pass over T and U of predict-with-gradients (the 10 lock-step L-BFGS seeds of solve_lbfgs fit in one)
constexpr int BM_SC_WORDS = 20;            // the words of the bound pass's sc[] (the last ones spare)
constexpr int BM_KS_MAX = 5;               // d + 2 <= 20: the candidates' fragments stay in registers (8 KS doubles per lane)
constexpr int TK_PER_THREAD = 16, TK_PER_BLOCK = 256 * TK_PER_THREAD;      // the device top-k's candidates per workgroup
constexpr int SEL_BINS = 4096, SEL_PER_THREAD = 16, SEL_PER_BLOCK = 256 * SEL_PER_THREAD;      // radix select / compaction
inline int64_t topk_blocks(int64_t M) { return (M + TK_PER_BLOCK - 1) / TK_PER_BLOCK; }
inline int64_t sel_blocks(int64_t M) { return (M + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK; }

struct WsRegion { const char* name; int64_t offset, bytes; };

// Walks one allocation from `base` (null: a sizing walk, every pointer null).  take() never pads: a region that would start off its
// element type's alignment is a bug in the walk, not something to adjust silently -- padding is spelled align_to() or skip().
class WsCarver {
    char* base_;
    int64_t off_ = 0;
    std::vector<WsRegion>* rec_;      // (the host check's record of the regions)
public:
    explicit WsCarver(void* base, std::vector<WsRegion>* rec = nullptr) : base_(static_cast<char*>(base)), rec_(rec) {}
    template <typename T> T* take(int64_t n, const char* name) {
        assert(n >= 0 && off_ % (int64_t)alignof(T) == 0);
        if (rec_) rec_->push_back({name, off_, n * (int64_t)sizeof(T)});
        char* p = base_ ? base_ + off_ : nullptr;
        off_ += n * (int64_t)sizeof(T);
        return reinterpret_cast<T*>(p);
    }
    template <typename T> void skip(int64_t n) { assert(n >= 0); off_ += n * (int64_t)sizeof(T); }
    void align_to(int64_t bytes) { off_ = (off_ + bytes - 1) / bytes * bytes; }
    int64_t bytes() const { return off_; }
};

// the host form of a sweep (h->dXc): the candidates, where given (nx = M d), and the three output vectors
struct StagedWs { double *X, *acq, *mu, *s2; int64_t bytes; };
inline StagedWs staged_ws(WsCarver c, int64_t nx, int64_t M) {
    return {c.take<double>(nx, "X"), c.take<double>(M, "acq"), c.take<double>(M, "mu"), c.take<double>(M, "s2"), c.bytes()};
}

// the ensemble sweep's accumulators and member outputs (h->dens)
struct EnsWs { double *acc0, *acc1, *t0, *t1, *out; int64_t bytes; };
inline EnsWs ens_ws(WsCarver c, int64_t M) {
    return {c.take<double>(M, "acc0"), c.take<double>(M, "acc1"), c.take<double>(M, "t0"), c.take<double>(M, "t1"), c.take<double>(M, "out"), c.bytes()};
}

// the constrained sweep's scratch (h->dcon): one constraint's probabilities of feasibility, and the running product where the caller
// gave no vector for it
struct ConWs { double *t0, *out; int64_t bytes; };
inline ConWs con_ws(WsCarver c, int64_t M) {
    return {c.take<double>(M, "t0"), c.take<double>(M, "out"), c.bytes()};
}

// the two-objective sweep's scratch (h->dehvi): the members' moments as k_ehvi_fold reads them ((4, M): mu1, s2_1, mu2, s2_2), the values
// where the caller gave no vector for them, and the strips of a front of n points (a_0 .. a_{n+1}, then b_0 .. b_n and one word of padding)
struct EhviWs { double *mom, *out, *a, *b; int64_t bytes; };
inline EhviWs ehvi_ws(WsCarver c, int64_t M, int64_t n) {
    double* const mom = c.take<double>(M, "mu1");
    c.take<double>(M, "s2_1"), c.take<double>(M, "mu2"), c.take<double>(M, "s2_2");
    return {mom, c.take<double>(M, "out"), c.take<double>(n + 2, "a"), c.take<double>(n + 2, "b"), c.bytes()};
}

// What the two-objective batch (gpx_ehvi_sweep_batch) adds to the lead's scratch (h->dehvib; nothing here grows with M): the strips at
// their capacity -- a then b, ld = EHVI_STRIP_LD doubles each, so that a front may grow in place and one upload fills both --, the picks'
// believed outcomes (64, 2), the size of the front that scored each pick, and the current size n, the word the scoring kernel reads
struct EhviBatchWs { double *a, *b, *y; int64_t* nfront; int* n; int64_t bytes; };
inline EhviBatchWs ehvi_batch_ws(WsCarver c, int64_t ld) {
    EhviBatchWs w = {c.take<double>(ld, "a"), c.take<double>(ld, "b"), c.take<double>(128, "sel_y"), c.take<int64_t>(64, "sel_nfront"),
                     c.take<int>(1, "n"), 0};
    c.skip<int>(1), w.bytes = c.bytes();
    return w;
}

// The matrix-pipe bound kernels' operands (kernels_sweep.hip: launch_bound_mfma), every one on a 32-byte boundary: the augmented rows
// in KS k-steps, the weights, the norms where they go through the accumulator (nc; KS <= 4 there), the centre at its fixed place, then
// the fp32 copies over Np + B32_ZROWS rows (W': the factorised walk's scaled weights).  Sized with KS = BM_KS_MAX, nc = false.
struct BoundOps { double *A, *W4, *NX4, *cen; float *A32, *W32, *WF32, *NX32; };
inline BoundOps bound_ops(WsCarver& c, int64_t Np, int KS, bool nc) {
    const int64_t Np32 = Np + B32_ZROWS;
    BoundOps b;
    b.A = c.take<double>(Np * 4 * KS, "A"), b.W4 = c.take<double>(Np, "W4");
    b.NX4 = nc ? c.take<double>(Np, "NX4") : nullptr;
    c.skip<double>(Np * 4 * (BM_KS_MAX - KS) - (nc ? Np : 0));      // the k-steps this d does not use
    b.cen = c.take<double>(4 * BM_KS_MAX, "cen");
    b.A32 = c.take<float>(Np32 * 4 * KS, "A32"), b.W32 = c.take<float>(Np32, "W32"), b.WF32 = c.take<float>(Np32, "WF32");
    b.NX32 = nc ? c.take<float>(Np32, "NX32") : nullptr;
    c.skip<float>(Np32 * (4 * (BM_KS_MAX - KS) + 2 - (nc ? 1 : 0)));      // ... and two spare rows' worth
    return b;
}

// The pruning workspace (h->dprune) of a selection-only sweep of M candidates with room for `cap` survivors: the bound vector, the
// seeds' / survivors' values, coordinates and indices, the compaction's block sums, the bound pass's weights, the gate's s2, sc[],
// `extra` words of the ensemble lead, the radix select's two histograms and state, the bound kernels' operands (bws); with `rows`
// (the single model's sweep) the second bound's dots, values, row sums, list and block sums.
struct PruneWs {
    double *ub, *vals, *Xg, *alpha2, *sabs, *gs2, *sc, *extra, *bws, *dots, *ub2, *qR, *Xg2;
    int64_t *idx, *blk, *idx2, *blk2, nsel, bytes;
    int *hist, *st;
};
inline PruneWs prune_ws_layout(WsCarver c, int64_t M, int64_t cap, int64_t d, int64_t Np, int64_t Gg, int64_t extra, bool rows) {
    PruneWs w = {};
    w.ub = c.take<double>(M, "ub"), w.vals = c.take<double>(cap, "vals"), w.Xg = c.take<double>(cap * d, "Xg");
    w.idx = c.take<int64_t>(cap, "idx"), w.blk = c.take<int64_t>((w.nsel = sel_blocks(M)) + 1, "blk");
    w.alpha2 = c.take<double>(Np, "alpha2"), w.sabs = c.take<double>(Np, "sabs"), w.gs2 = c.take<double>(Gg, "gs2");
    w.sc = c.take<double>(BM_SC_WORDS, "sc"), w.extra = c.take<double>(extra, "extra");
    w.hist = c.take<int>(2 * SEL_BINS, "hist"), w.st = c.take<int>(8, "st");
    c.align_to(32), w.bws = bound_ops(c, Np, BM_KS_MAX, false).A;
    if (rows) {
        w.dots = c.take<double>(M, "dots"), w.ub2 = c.take<double>(cap, "ub2"), w.qR = c.take<double>(cap, "qR");
        w.idx2 = c.take<int64_t>(cap, "idx2"), w.Xg2 = c.take<double>(cap * d, "Xg2"), w.blk2 = c.take<int64_t>(sel_blocks(cap) + 1, "blk2");
    }
    w.bytes = c.bytes();
    return w;
}

// option prune_keep (h->dkeep): the bound vector and the seed list as they were before the scatter, the dots as the kernel left them
struct KeepWs { double* ub; int64_t* seed; double* dots; int64_t bytes; };
inline KeepWs keep_ws(WsCarver c, int64_t M, int64_t G) {
    return {c.take<double>(M, "ub"), c.take<int64_t>(G, "seed"), c.take<double>(M, "dots"), c.bytes()};
}

// queued cache corrections (h->dpend): PEND_MAX weight rows of pitch ld, then {1/d, a_new} per row
struct PendWs { double *rows, *scal; int64_t bytes; };
inline PendWs pend_ws(WsCarver c, int64_t ld) {
    return {c.take<double>(PEND_MAX * ld, "rows"), c.take<double>(PEND_MAX * 2, "scal"), c.bytes()};
}

// gpx_append's scratch (h->dgrad): the point padded to xpad, then what launch_append_prepare writes
struct AppendWs { double *x, *ks, *g, *r, *tu; int64_t bytes; };
inline AppendWs append_ws(WsCarver c, int64_t xpad, int64_t Np) {
    return {c.take<double>(xpad, "x"), c.take<double>(Np, "ks"), c.take<double>(Np, "g"), c.take<double>(Np, "r"), c.take<double>(Np, "tu"), c.bytes()};
}

// what an announced append and a batch pick's conditioning share: the point raw and scaled (xpad each), launch_append_prepare's four
// vectors and the weight row, all of pitch ld
struct SpecFront { double *x, *xs, *ks, *g, *r, *tu, *row; };
inline SpecFront spec_front(WsCarver& c, int64_t xpad, int64_t ld) {
    return {c.take<double>(xpad, "x"), c.take<double>(xpad, "xs"), c.take<double>(ld, "ks"), c.take<double>(ld, "g"),
            c.take<double>(ld, "r"), c.take<double>(ld, "tu"), c.take<double>(ld, "row")};
}

// the announcement (h->dspec): the front, its scalars, and its row of V over the M cached candidates on a 512-byte boundary
struct SpecBuf : SpecFront { double *pscal, *scal, *v; int64_t bytes; };
inline SpecBuf spec_ws(WsCarver c, int64_t xpad, int64_t ld, int64_t M) {
    SpecBuf b = {spec_front(c, xpad, ld), c.take<double>(2, "pscal"), c.take<double>(16, "scal"), nullptr, 0};
    c.skip<double>(46);              // keeps v 512-byte aligned (2 + 16 + 46 = 64 doubles)
    b.v = c.take<double>(M, "v"), b.bytes = c.bytes();
    return b;
}

// Batch proposals (h->dbsel; one per member of gpx_ensemble_sweep_batch): the front with ld = capacity + NB, the picks' small state in
// slots of 8 / 16 / 64 doubles (pscal {1/d, 0}; scal_prep the prepare's scalars, unused; scal {d, 1/d, 0, d^2}; flag its flag word; same
// the lead's same-grid word), the argmax partials, q' and s2, the taken bytes, nb rows of V, the lead's sel_s2 (n_lead x nb) and descriptors
struct BatchBuf : SpecFront {
    double *pscal, *scal_prep, *scal, *cross, *sel_val, *sel_s2, *partv, *qp, *s2, *V, *ens_s2, *desc;
    int *flag, *same;
    int64_t *sel_idx, *parti, ld, ntaken, bytes;
    unsigned char* taken;
};
inline BatchBuf batch_ws(WsCarver c, int64_t xpad, int64_t ld, int64_t M, int64_t nb, int64_t n_lead, int64_t ndesc) {
    BatchBuf b = {};
    static_cast<SpecFront&>(b) = spec_front(c, xpad, ld);
    b.ld = ld, b.ntaken = (M + 7) / 8;
    b.pscal = c.take<double>(8, "pscal"), b.scal_prep = c.take<double>(16, "scal_prep"), b.scal = c.take<double>(16, "scal");
    b.flag = c.take<int>(1, "flag"), c.skip<int>(15), b.same = c.take<int>(1, "same"), c.skip<int>(31);
    b.cross = c.take<double>(64, "cross"), b.sel_val = c.take<double>(64, "sel_val"), b.sel_s2 = c.take<double>(64, "sel_s2");
    b.sel_idx = c.take<int64_t>(64, "sel_idx"), c.skip<double>(64);      // (spare)
    b.partv = c.take<double>(1024, "partv"), b.parti = c.take<int64_t>(1024, "parti");
    b.qp = c.take<double>(M, "qp"), b.s2 = c.take<double>(M, "s2"), b.taken = c.take<unsigned char>(b.ntaken * 8, "taken");
    b.V = c.take<double>(nb * M, "V"), b.ens_s2 = c.take<double>(n_lead * nb, "ens_s2"), b.desc = c.take<double>(ndesc, "desc");
    b.bytes = c.bytes();
    return b;
}

// Fantasised batch proposals (h->dfant; the per-candidate state is the believer's BatchBuf, so nothing here grows with M): the
// innovations eps[l][s] pick-major over max(nb - 1, 1) rows of pitch Sp = S rounded up to the scoring kernel's chunk of FANT_CHUNK
// fantasies (padding: zeros), so that a round's rows are one contiguous copy into LDS and a chunk one aligned run; the incumbents
// t[Sp]; the forced rows of the leading rounds.
constexpr int FANT_CHUNK = 16, FANT_MAX_S = 64;
struct FantWs { double *eps, *t; int64_t* pend; int64_t Sp, bytes; };
inline FantWs fant_ws(WsCarver c, int64_t nb, int64_t S) {
    const int64_t Sp = (S + FANT_CHUNK - 1) / FANT_CHUNK * FANT_CHUNK, rows = nb > 1 ? nb - 1 : 1;
    return {c.take<double>(rows * Sp, "eps"), c.take<double>(Sp, "t"), c.take<int64_t>(64, "pend_idx"), Sp, c.bytes()};
}

// predict with gradients (h->dgrad): GB points, per point k*, its gradient panel, V, w over Np rows, `per` = 2 + 2 d outputs, and the
// register-blocked matvec's nseg segment partials
struct GradWs { double *X, *ks, *g, *V, *w, *out, *part; int64_t bytes; };
inline GradWs grad_ws(WsCarver c, int64_t d, int64_t Np, int64_t nseg) {
    return {c.take<double>(GB * d, "X"), c.take<double>(GB * Np, "ks"), c.take<double>(GB * Np, "g"), c.take<double>(GB * Np, "V"),
            c.take<double>(GB * Np, "w"), c.take<double>(GB * (2 + 2 * d), "out"), c.take<double>(nseg * GB * Np, "part"), c.bytes()};
}

// gpx_rff_grad (h->dgrad): one draw's parameters, the points, [f, df/dx] per point
struct RffGradWs { double *W, *b, *th, *X, *out; int64_t bytes; };
inline RffGradWs rff_grad_ws(WsCarver c, int64_t n, int64_t d, int64_t M) {
    return {c.take<double>(n * d, "W"), c.take<double>(n, "b"), c.take<double>(n, "th"), c.take<double>(M * d, "X"), c.take<double>(M * (d + 1), "out"), c.bytes()};
}

// The joint posterior at M points, Mp padded (h->djoint), every part up to R on a 256-byte boundary: the points, scaled, the mean and
// its nP partial rows, V = T Ks panel-major, Kss, C; for draws B, its factor R, the normals and the S draws.
struct JointWs { double *X, *Zs, *mu, *Pp, *V, *Kss, *C, *B, *R, *z, *out; int64_t bytes; };
inline JointWs joint_ws(WsCarver c, int64_t M, int64_t Mp, int64_t d, int64_t nP, int64_t Np, bool draw, int64_t S) {
    double* const X = c.take<double>(M * d, "X");
    c.align_to(256);
    return {X, c.take<double>(Mp * d, "Zs"), c.take<double>(Mp, "mu"), c.take<double>(nP * Mp, "Pp"), c.take<double>(Np * Mp, "V"),
            c.take<double>(Mp * Mp, "Kss"), c.take<double>(Mp * Mp, "C"), draw ? c.take<double>(Mp * Mp, "B") : nullptr,
            draw ? c.take<double>(Mp * Mp, "R") : nullptr, draw ? c.take<double>(S * M, "z") : nullptr, draw ? c.take<double>(S * M, "out") : nullptr, c.bytes()};
}

// the prepared support set (h->dkg): the set raw and scaled, its means a_j, B, V_A and the means' partial rows
struct KgBuf { double *A, *As, *al, *B, *V, *Pp; int m; int64_t bytes; };
inline KgBuf kg_ws(WsCarver c, int64_t d, int64_t Np, int m) {
    return {c.take<double>(NB * d, "A"), c.take<double>(NB * d, "As"), c.take<double>(NB, "al"), c.take<double>(Np * NB, "B"),
            c.take<double>(Np * NB, "V"), c.take<double>(Np / NB * NB, "Pp"), m, c.bytes()};
}

// gpx_kg_grad's panels of 128 points (h->dkgw): the Mp padded points, V_z, W_z, the sums S, the lines' scratch L, value and gradient
struct KgPointWs { double *Z, *Vz, *Wz, *S, *L, *f, *g; int64_t bytes; };
inline KgPointWs kg_point_ws(WsCarver c, int64_t Mp, int64_t d, int64_t Np) {
    return {c.take<double>(Mp * d, "Z"), c.take<double>(Np * NB, "Vz"), c.take<double>(Np * NB, "Wz"), c.take<double>((int64_t)NB * (d + 1) * 132, "S"),
            c.take<double>(4 * (int64_t)(KG_MAX_LINES + 1) * NB, "L"), c.take<double>(Mp, "f"), c.take<double>(Mp * d, "g"), c.bytes()};
}

// the re-tiled draw parameters of a Thompson sweep
struct RffSweepWs { double *Wt, *bt, *tt; int64_t bytes; };
inline RffSweepWs rff_sweep_ws(WsCarver c, int64_t nW, int64_t nV) {
    return {c.take<double>(nW, "Wt"), c.take<double>(nV, "bt"), c.take<double>(nV, "tt"), c.bytes()};
}

// feature Grams of S draws of n < 128 features: the tiles and phases, A (S, n, n), v (S, n), `extra` doubles for the caller
struct RffGramWs { double *Wt, *bt, *A, *v, *extra; int64_t bytes; };
inline RffGramWs rff_gram_ws(WsCarver c, int64_t nW, int64_t nV, int64_t S, int64_t n, int64_t extra) {
    return {c.take<double>(nW, "Wt"), c.take<double>(nV, "bt"), c.take<double>(S * n * n, "A"), c.take<double>(S * n, "v"), c.take<double>(extra, "extra"), c.bytes()};
}

// wide feature maps (n >= 128), one draw at a time: its parameters, Gram and vector, for the posterior (p) the normals, work, theta,
// B and its factor over np padded features, and the feature slab Ft
struct RffWideWs { double *W, *b, *A, *v, *z, *work, *th, *B, *R, *Ft; int64_t bytes; };
inline RffWideWs rff_wide_ws(WsCarver c, int64_t n, int64_t d, int64_t np, int64_t Np, bool p) {
    RffWideWs w = {c.take<double>(n * d, "W"), c.take<double>(n, "b"), c.take<double>(n * n, "A"), c.take<double>(n, "v"), p ? c.take<double>(n, "z") : nullptr,
                   p ? c.take<double>(n, "work") : nullptr, p ? c.take<double>(n, "th") : nullptr, p ? c.take<double>(np * np, "B") : nullptr,
                   p ? c.take<double>(np * np, "R") : nullptr, c.take<double>(n * Np, "Ft"), 0};
    if (p) c.skip<double>(n);        // slack the allocation has always had
    w.bytes = c.bytes();
    return w;
}

// Pathwise Thompson draws (h->dpath; kernels_path.hip).  The weight panel of a sweep in the fragment order of v_mfma_f64_16x16x4:
// per group of at most PATH_GROUP draws, per 64-row tile of the leading nv observations, per k-step of 4 rows, one 64-lane fragment
// for each block of 16 draws the group holds (rows >= nv and draws >= S: zeros).
constexpr int PATH_GROUP = 64, PATH_ROWS = 64;
inline int64_t path_tiles(int64_t nv) { return (nv + PATH_ROWS - 1) / PATH_ROWS; }
inline int path_group_blocks(int64_t S, int64_t g) { return (int)((std::min<int64_t>(PATH_GROUP, S - g * PATH_GROUP) + 15) / 16); }
inline int64_t path_group_offset(int64_t nv, int64_t g) { return g * path_tiles(nv) * (PATH_ROWS / 4) * (PATH_GROUP / 16) * 64; }      // (every earlier group is full)
inline int64_t path_frag_words(int64_t S, int64_t nv) {
    const int64_t G = (S + PATH_GROUP - 1) / PATH_GROUP;
    return path_group_offset(nv, G - 1) + path_tiles(nv) * (PATH_ROWS / 4) * path_group_blocks(S, G - 1) * 64;
}
// gpx_path_sweep: the caller's weights (S, nv) as uploaded, then the panel on a 512-byte boundary
struct PathSweepWs { double *v, *frag; int64_t bytes; };
inline PathSweepWs path_sweep_ws(WsCarver c, int64_t S, int64_t nv) {
    double* const v = c.take<double>(S * nv, "v");
    c.align_to(512);
    return {v, c.take<double>(path_frag_words(S, nv), "frag"), c.bytes()};
}
// gpx_path_weights: the prior draws at the N observations (S, N), the caller's noise normals, the right-hand sides, T r and U T r as
// k-major panels of 128 draws [Sp / 128][Np][128] (every panel on a 512-byte boundary: Np 128 doubles each), the weights (S, N)
struct PathWeightsWs { double *prior, *eps, *R, *V, *W, *v; int64_t bytes; };
inline PathWeightsWs path_weights_ws(WsCarver c, int64_t S, int64_t N, int64_t Np, int64_t Sp, bool eps) {
    double* const prior = c.take<double>(S * N, "prior");
    double* const e = eps ? c.take<double>(S * N, "eps") : nullptr;
    c.align_to(512);
    return {prior, e, c.take<double>(Np * Sp, "R"), c.take<double>(Np * Sp, "V"), c.take<double>(Np * Sp, "W"), c.take<double>(S * N, "v"), c.bytes()};
}
// gpx_path_grad (h->dpath): one draw's parameters and leading weights, the M points, per pass of GB points k* and dk/dr2 over Np rows
// and k_mean_reduce's 2 + 2 d outputs per point, then [f, df/dx] per point
struct PathGradWs { double *W, *b, *th, *v, *X, *ks, *g, *part, *out; int64_t bytes; };
inline PathGradWs path_grad_ws(WsCarver c, int64_t n, int64_t d, int64_t nv, int64_t Np, int64_t M) {
    return {c.take<double>(n * d, "W"), c.take<double>(n, "b"), c.take<double>(n, "th"), c.take<double>(nv, "v"), c.take<double>(M * d, "X"),
            c.take<double>(GB * Np, "ks"), c.take<double>(GB * Np, "g"), c.take<double>(GB * (2 + 2 * d), "part"), c.take<double>(M * (d + 1), "out"), c.bytes()};
}

// gpx_loglik_batch (h->dbatch), B vectors at once: Gram, factor, scaled inputs, a, {rho, sn2, bias}, 1 / ell, the results, and for
// large factors the running right-hand sides and {a.a, sum log R_ii}; one flag word each
struct LoglikBatchWs { double *S, *R, *Xs, *a, *hyp, *invell, *out, *r, *acc; int* flag; int64_t bytes; };
inline LoglikBatchWs loglik_batch_ws(WsCarver c, int64_t B, int64_t Np, int64_t d) {
    LoglikBatchWs w = {c.take<double>(B * Np * Np, "S"), c.take<double>(B * Np * Np, "R"), c.take<double>(B * Np * d, "Xs"), c.take<double>(B * Np, "a"),
                       c.take<double>(3 * B, "hyp"), c.take<double>(B * DMAX, "invell"), c.take<double>(B, "out"), c.take<double>(B * Np, "r"),
                       c.take<double>(2 * B, "acc"), c.take<int>(B, "flag"), 0};
    c.align_to(8), c.skip<double>(8);      // (slack the allocation has always had)
    w.bytes = c.bytes();
    return w;
}

// gpx_loglik_grad (h->dhyper): d + 2 partial sums per tile, then [L, d + 3 components]
struct HyperWs { double *part, *res; int64_t bytes; };
inline HyperWs hyper_ws(WsCarver c, int64_t ntiles, int64_t d) {
    return {c.take<double>(ntiles * (d + 2), "part"), c.take<double>(d + 4, "res"), c.bytes()};
}

}  // namespace gpx
